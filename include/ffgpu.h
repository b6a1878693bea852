/*
 * ffgpu.h -- C ABI of libffgpu.so, the MI355X (gfx950) finite-field /
 * secret-sharing engine that sits behind MPyC's field-array and threshold
 * sharing interfaces.
 *
 * The reference (lschoe/mpyc) is pure Python and has no FFI of its own; the
 * seams this ABI plugs into are listed per entry point below as
 * "replaces: <reference file>:<lines>" (paths relative to the mpyc checkout).
 * INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every entry point returns an int status (FFGPU_OK == 0); nothing throws
 *     across the boundary.  ffgpu_strerror() maps a status to text; the Python
 *     shim maps statuses to the exceptions the reference raises.
 *   - all array arguments are DEVICE pointers unless the name says host.
 *     Elements are fixed-width little-endian limbs in canonical form
 *     (0 <= x < modulus; for GF(2^n) the bit pattern of the polynomial):
 *         elem_bytes == 1   GF(2^n), n <= 8           uint8  [n]
 *         elem_bytes == 4   prime p < 2^32, GF(2^n) 9 <= n <= 32   uint32 [n]
 *         elem_bytes == 8   prime p < 2^64, GF(2^n) 33 <= n <= 64  uint64 [n]
 *         elem_bytes == 12  prime p = 2^k - c, 65 <= k <= 96, c < 2^31   3 x uint32 (12-byte LE integer)
 *         elem_bytes == 16  other primes p < 2^128, GF(2^n) n<=128 {lo,hi} uint64 pairs
 *         elem_bytes == 24  primes of 129..192 bits            3 x uint64 (24-byte LE integer, 8-byte aligned)
 *     This is exactly the byte layout of field.to_bytes() (finfields.py:91-102)
 *     for byte_length in {1,4,8,12,16,24} (shorter byte_lengths are zero-padded to the storage width).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *     Calls are asynchronous on that stream; nothing synchronises unless the
 *     name says so.
 *   - inputs are never written; `out` may alias an input of the same shape for
 *     the element-wise entry points (in-place operators, finfields.py:1068-1124):
 *     ffgpu_reduce, ffgpu_add, ffgpu_sub, ffgpu_mul, ffgpu_neg, ffgpu_add_scalar,
 *     ffgpu_mul_scalar, ffgpu_rsub_scalar, ffgpu_muladd, ffgpu_pow, ffgpu_inv and
 *     ffgpu_beaver_combine.  Inputs may also alias each other (a == b).  Exact
 *     alias only; partial overlap is undefined.  Elements are canonical on return
 *     (tests/test_gpu_elementwise_contract.py).
 *   - share generation, the fused gate and recombination (ffgpu_split, ffgpu_mul_split, ffgpu_rng_coeffs,
 *     ffgpu_split_rng, ffgpu_mul_split_rng, ffgpu_split_rng_state, ffgpu_gate_rng, ffgpu_gate_rng_batch,
 *     ffgpu_recombine): inputs are never written, and nothing outside the n elements of each output row is
 *     written -- not the padding between n and the row stride, not a pack or a wave rounded up past a row's end.
 *     Any row stride >= n is allowed, whatever its alignment (strides and bases that keep rows 16-byte aligned take
 *     the vector paths; the result is the same).  Overlap: ffgpu_recombine with w == 1 may have `out` be EXACTLY one
 *     of its rows (every route loads an element of all rows before it stores that element); partial overlap is
 *     undefined.  For w > 1, and for every share-generation and gate call, the output block (all its rows, padding
 *     included) must not overlap any input: rows are re-read per output row.  Elements are canonical on return
 *     (tests/test_gpu_share_contract.py).
 *   - thread-safety: the field description of a context is immutable after
 *     creation and a context may be shared between host threads and streams;
 *     its only mutable state -- the ffgpu_matmul scratch buffers (one per
 *     stream, under a mutex) and the lazily built tables -- is internally
 *     synchronised.  Two host threads must not issue work on the SAME stream
 *     of a context concurrently.  The reference only ever calls from one
 *     event-loop thread (asyncoro.py:416-464).
 */
#ifndef FFGPU_H
#define FFGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FFGPU_ABI_VERSION 1

/* status codes */
#define FFGPU_OK          0
#define FFGPU_EINVAL      1   /* bad argument (null pointer, t >= m, k == 0, ...)   */
#define FFGPU_ENOTSUP     2   /* field / size outside what this build supports      */
#define FFGPU_EHIP        3   /* a HIP runtime call failed; see ffgpu_last_hip_error */
#define FFGPU_EMODULUS    4   /* modulus is not usable (even/zero/one, too wide)     */
#define FFGPU_ENOMEM      5
#define FFGPU_ESTALE      6   /* ffgpu_ipc_read: the mapping does not show the row the descriptor describes */

/* field kinds */
#define FFGPU_PRIME   1   /* GF(p), p prime < 2^192       (finfields.py:347-363 pGF)  */
#define FFGPU_BINARY  2   /* GF(2^n), 1 <= n <= 128       (finfields.py:508-525 xGF,
                             gfpx.py:848-1121 BinaryPolynomial)                       */

/* reduction strategy picked at context creation (reported for logs/tests) */
#define FFGPU_RED_PSEUDO_MERSENNE 1  /* p = 2^k - c, small c: fold reduction          */
#define FFGPU_RED_RECIPROCAL      2  /* arbitrary modulus: Barrett-type reciprocal    */
#define FFGPU_RED_GF2_SWAR        3  /* GF(2^n), n<=8: packed shift-xor               */
#define FFGPU_RED_GF2_WIDE        4  /* GF(2^n), n<=128: limb shift-xor               */
#define FFGPU_RED_MONTGOMERY      5  /* arbitrary odd 65..192-bit p: word-serial REDC */

typedef struct ffgpu_ctx ffgpu_ctx;

/* ---- library / device ------------------------------------------------- */
int         ffgpu_abi_version(void);
const char* ffgpu_strerror(int status);
const char* ffgpu_last_hip_error(void);          /* text of the last failing HIP call */
int         ffgpu_device_count(int* count);
/* PCI bus id ("0000:05:00.0") of a device into buf (len >= 16): lets a multi-process run show that its ranks sit on
 * distinct GPUs.  No reference counterpart (the reference has no device).                                          */
int         ffgpu_device_pci_bus_id(int device, char* buf, int len);

/* ---- field context ---------------------------------------------------- */
/* modulus: little-endian uint64 limbs.  FFGPU_PRIME: the prime p, nlimbs 1..3: primes of 129..192 bits are stored
 * as three 64-bit limbs = 24 bytes per element (p = 2^k - c with c < 2^31 -- the l+32-bit default fields of
 * SecInt(97..160), sectypes.py:673-676 -- reduce by folding, any other odd prime of that size -- e.g. the
 * root-of-unity primes of SecInt(l, n=N), finfields.py:332-343 -- by Montgomery products); above 192 bits:
 * FFGPU_ENOTSUP.
 * FFGPU_BINARY: bit pattern of the irreducible polynomial including its leading
 * term (degree n <= 128 needs up to 3 limbs).  Primality / irreducibility is the
 * caller's job (the reference checks it in pGF/xGF before any array exists).
 * replaces: finfields.py:23-60 (GF / arrayGF pick the array representation). */
int ffgpu_ctx_create(int kind, const uint64_t* modulus, int nlimbs, int device,
                     ffgpu_ctx** out);
int ffgpu_ctx_destroy(ffgpu_ctx* ctx);
/* Opt-in timing: with enable != 0 every compute call records a pair of events on its stream around the
 * kernels it launches; ffgpu_last_kernel_ms waits for the most recent call and returns its GPU time
 * (FFGPU_EINVAL if timing is off or nothing has been launched).  Off by default: no events, no cost.   */
int ffgpu_ctx_set_timing(ffgpu_ctx* ctx, int enable);
int ffgpu_last_kernel_ms(ffgpu_ctx* ctx, float* ms);
/* enable == 2: ACCUMULATE -- every compute call keeps its own event pair; ffgpu_busy_ms waits for the calls issued so
 * far and returns the summed GPU time of all calls since the last reset (and their number): the "GPU busy" numerator
 * of an API-level measurement (bench.py `api`).  Calls on one stream do not overlap, so the sum is busy time.        */
int ffgpu_busy_ms(ffgpu_ctx* ctx, double* ms, unsigned long long* calls, int reset);
int ffgpu_ctx_elem_bytes(const ffgpu_ctx* ctx);   /* 1, 4, 8, 12, 16 or 24       */
/* Host SCALARS (constants, Lagrange coefficients, matrix entries, PRSS weights: every `const uint64_t* host_...`
 * argument that is documented as "canonical 2-limb scalars") occupy ffgpu_ctx_scalar_limbs(ctx) little-endian
 * limbs each: 2, or 3 for the 24-byte prime fields.  Exponents (ffgpu_pow) may have up to 3 limbs.            */
int ffgpu_ctx_scalar_limbs(const ffgpu_ctx* ctx);
int ffgpu_ctx_reduction(const ffgpu_ctx* ctx);    /* one of FFGPU_RED_*          */
int ffgpu_ctx_device(const ffgpu_ctx* ctx);

/* ---- device memory (optional: any hipMalloc'ed / torch pointer works) -- */
int ffgpu_malloc(ffgpu_ctx* ctx, size_t bytes, void** dptr);
int ffgpu_free(ffgpu_ctx* ctx, void* dptr);
int ffgpu_h2d(ffgpu_ctx* ctx, void* dst, const void* host_src, size_t bytes, void* stream);
int ffgpu_d2h(ffgpu_ctx* ctx, void* host_dst, const void* src, size_t bytes, void* stream);
int ffgpu_stream_sync(ffgpu_ctx* ctx, void* stream);

/* ---- canonical reduction ---------------------------------------------- */
/* out[i] = raw[i] mod modulus for arbitrary limb patterns of elem_bytes width.
 * replaces: finfields.py:717-725 (`value %= modulus` in FiniteFieldArray.__init__) */
int ffgpu_reduce(ffgpu_ctx* ctx, const void* raw, void* out, size_t n, void* stream);

/* ---- element-wise field arithmetic, arrays of equal length n ---------- */
/* replaces: finfields.py:1056-1103 (__add__/__sub__/__iadd__/__isub__),
 *           :1105-1124 (__mul__/__imul__), :1189-1192 (__neg__);
 *           GF(2^n): gfpx.py:982-1045 (_add/_mul/_mod).                      */
int ffgpu_add(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream);
int ffgpu_sub(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream);
int ffgpu_mul(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n, void* stream);
int ffgpu_neg(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* stream);

/* array (op) scalar; scalar is a HOST value in canonical limbs (2 x uint64,
 * little-endian, upper limb 0 for narrow fields).
 * replaces: the `other` is int / field element branch of finfields.py:1045-1054. */
int ffgpu_add_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* host_scalar, void* out, size_t n, void* stream);
int ffgpu_mul_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* host_scalar, void* out, size_t n, void* stream);
/* out = scalar - a   (finfields.py:1084-1091 __rsub__)                        */
int ffgpu_rsub_scalar(ffgpu_ctx* ctx, const void* a, const uint64_t* host_scalar, void* out, size_t n, void* stream);

/* out = a * b + c   (fused multiply-add; one pass instead of two)            */
int ffgpu_muladd(ffgpu_ctx* ctx, const void* a, const void* b, const void* c, void* out, size_t n, void* stream);

/* ---- second-tier element-wise operations -------------------------------- */
/* out[i] = a[i]^e for a public exponent e >= 0 (little-endian uint64 limbs, exp_limbs <= 2).
 * One pass: square-and-multiply in registers.
 * replaces: finfields.py:1159-1187 (__pow__), :1408-1414 (_pow via gmpy2.powmod per element);
 * sqrt for p = 3 mod 4 is pow by (p+1)/4 (:1424-1458), Legendre symbol pow by (p-1)/2 (:1460-1470). */
int ffgpu_pow(ffgpu_ctx* ctx, const void* a, const uint64_t* host_exp, int exp_limbs, void* out, size_t n,
              void* stream);
/* out[i] = a[i]^-1.  Batched with Montgomery's trick inside each thread (3 products per element
 * plus one exponentiation per 16..128 elements).  a[i] == 0 gives out[i] = 0 and ORs 1 into
 * *dev_zero_flag (device int32, may be NULL): the reference raises ZeroDivisionError there
 * (gmpy.py:197-210), which the host wrapper does after reading the flag.
 * replaces: finfields.py:1278-1281 (reciprocal), :1416-1422 (_reciprocal via gmpy2.invert per element). */
int ffgpu_inv(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* dev_zero_flag, void* stream);

/* ---- Beaver-triple combination (NOT a reference function; parity UNPINNED) ------------- */
/* out = z + d*y + e*x (+ d*e if add_de != 0), element-wise: the local step of Beaver multiplication
 * after d = a - x and e = b - y have been opened ([x],[y],[z] = shares of a triple z = x*y).  add_de:
 * whether this party adds the public term d*e -- every party under Shamir sharing (a public constant is
 * shared by the constant polynomial), exactly one party under additive sharing.  MPyC itself multiplies with GRR resharing (runtime.py:603-689) and
 * has no Beaver triples; this entry point exists because the project brief names
 * it and is validated only against the textbook identity, not against reference outputs.          */
int ffgpu_beaver_combine(ffgpu_ctx* ctx, const void* z, const void* x, const void* y, const void* d,
                         const void* e, int add_de, void* out, size_t n, void* stream);

/* ---- Shamir share generation ------------------------------------------ */
/* shares[i][h] = secrets[h] + sum_{j<t} coeffs[j][h] * (i+1)^(j+1)  (mod modulus),
 * i = 0..m-1, h = 0..n-1;  coeffs is (t, n) row-major with row stride
 * coeff_stride elements, shares is (m, n) row-major with row stride
 * share_stride elements (strides let callers keep rows 16-byte aligned).
 * For GF(2^n) the x-coordinate of party i is the polynomial with bit pattern i+1.
 * This is the np-path coefficient convention: coeffs[j] multiplies X^(j+1).
 * replaces: thresha.py:47-64 np_random_split (C drawn at :60, V @ [s;C] at :61-63).
 * The list path thresha.py:23-44 random_split is the same map with
 * coeffs[j][h] = c_h[t-1-j].                              */
int ffgpu_split(ffgpu_ctx* ctx, const void* secrets, const void* coeffs, size_t coeff_stride,
                int t, int m, void* shares, size_t share_stride, size_t n, void* stream);

/* Fused local product + share generation: secrets[h] = a[h]*b[h] is never
 * written to memory.
 * replaces: runtime.py:1134-1138 (c = a * b; c = self._reshare(c)) up to the
 * send at runtime.py:661-667.                                                  */
int ffgpu_mul_split(ffgpu_ctx* ctx, const void* a, const void* b, const void* coeffs,
                    size_t coeff_stride, int t, int m, void* shares, size_t share_stride,
                    size_t n, void* stream);

/* ---- share generation with the on-device CSPRNG ------------------------- */
/* Same maps as ffgpu_split / ffgpu_mul_split, but the t*n coefficients are drawn inside the
 * kernel from a ChaCha keystream (host_key32: 32 bytes from the host CSPRNG, fresh per call or
 * with a fresh nonce; rounds: 20, 12 or 8; 0 = 20) and never touch HBM.  The keystream layout and
 * the 2^-64-bias field sampler are documented in mpyc_amd/csrc/rng.hpp; ffgpu_rng_coeffs writes
 * exactly the coefficient matrix the fused kernels consume for the same (key, nonce, rounds, t),
 * so split_rng(key) == split(rng_coeffs(key)) bit for bit.
 * replaces: the secrets.randbelow draws of thresha.py:37 and :58-60 (one OS-CSPRNG call per
 * coefficient in the reference).                                                            */
int ffgpu_rng_coeffs(ffgpu_ctx* ctx, const uint8_t* host_key32, uint64_t nonce, int rounds, int t,
                     void* coeffs, size_t coeff_stride, size_t n, void* stream);
int ffgpu_split_rng(ffgpu_ctx* ctx, const void* secrets, const uint8_t* host_key32, uint64_t nonce,
                    int rounds, int t, int m, void* shares, size_t share_stride, size_t n, void* stream);
int ffgpu_mul_split_rng(ffgpu_ctx* ctx, const void* a, const void* b, const uint8_t* host_key32,
                        uint64_t nonce, int rounds, int t, int m, void* shares, size_t share_stride,
                        size_t n, void* stream);

/* Fused chain gate: shares[i][h] = share of (A[h] * B[h]) for party i+1 where BOTH factors are given as
 * recombinations, A[h] = sum_j lambda_a[j] * rows_a[j][h] (ka <= 7 rows) and B likewise (kb = 0: B = A, a
 * squaring; a factor that already exists as an array is the 1-row case with lambda = 1).  One pass: recombine
 * in registers, multiply, draw the degree-t coefficients from the device CSPRNG (dev_state != NULL: the
 * device-resident state, else host key / nonce / rounds), write the m share rows.  In a chain of secure
 * multiplications this is `np_recombine` of the previous gate (thresha.py:119-132) + the local product and
 * `np_random_split` of the next one (runtime.py:1134-1138, thresha.py:47-64) without the recombined share
 * ever going to HBM: 6 instead of 9 memory accesses per element for a squaring.  t <= 3, else FFGPU_ENOTSUP
 * (callers then use ffgpu_recombine + ffgpu_mul_split_rng).  lambda: canonical 2-limb host scalars.          */
int ffgpu_gate_rng(ffgpu_ctx* ctx, const void* const* host_rows_a, const uint64_t* host_lambda_a, int ka,
                   const void* const* host_rows_b, const uint64_t* host_lambda_b, int kb, const uint8_t* host_key32,
                   uint64_t nonce, int rounds, void* dev_state, int t, int m, void* shares, size_t share_stride,
                   size_t n, void* stream);

/* `nbatch` independent chain gates in ONE launch (grid rows): gate y reads every row of A at element offset
 * y * batch_stride_a (B: y * batch_stride_b) from the given row pointers and writes its m share rows at
 * shares + y * batch_stride_out (+ i * share_stride for party i+1); its coefficients come from the call's
 * generator stream with y added to bits 8..15 of nonce word 1 (nbatch <= 255), so the gates draw independent
 * randomness (dev_state / nonce / defer_advance: see ffgpu_rng_state_advance below).  Bits 40..47 of `nonce` are
 * therefore RESERVED for the batch row on the host-key path: nbatch > 1 requires nonce < 2^40 (FFGPU_EINVAL
 * otherwise), so that (key, nonce, row) never aliases (key, nonce', row') under a reused key.  This is what the 2t+1 re-sharing parties of one `_reshare` (runtime.py:658-666) do when a whole
 * computation is held on one GPU: with the sub-shares stored [recipient][sender][n] the senders of the next gate
 * are batch_stride = (2t+1)*n apart and a layer of the np_aes S-box chain (runtime.py:1356-1367) is one launch
 * instead of 2t+1.  nbatch = 1 is ffgpu_gate_rng.                                                              */
int ffgpu_gate_rng_batch(ffgpu_ctx* ctx, const void* const* host_rows_a, const uint64_t* host_lambda_a, int ka,
                         size_t batch_stride_a, const void* const* host_rows_b, const uint64_t* host_lambda_b, int kb,
                         size_t batch_stride_b, const uint8_t* host_key32, uint64_t nonce, int rounds, void* dev_state,
                         int defer_advance, int t, int m, void* shares, size_t share_stride, size_t batch_stride_out,
                         size_t n, int nbatch, void* stream);

/* Deferred advance of a device-resident generator state: with dev_state != NULL, ffgpu_gate_rng_batch draws from
 * (state nonce + `nonce`) -- `nonce` < 2^32 is then an OFFSET -- and, if defer_advance != 0, leaves the state alone.
 * A sequence of N launches uses offsets 0..N-1 and ends with ONE ffgpu_rng_state_advance(state, N), instead of one
 * nonce update (a one-thread kernel for large grids, ~4 us) after every launch; captured in a HIP graph the offsets
 * are constants and the single advance keeps every replay on fresh nonces.                                        */
int ffgpu_rng_state_advance(ffgpu_ctx* ctx, void* dev_state, uint32_t by, void* stream);

/* Device-resident generator state, for launches captured in a HIP graph: the kernels read key / nonce /
 * rounds from `dev_state` (ffgpu_rng_state_bytes() bytes of device memory) when they start, and the nonce is
 * advanced on the device after every use (by the last workgroup of the share-generation kernel itself), so each REPLAY of a captured ffgpu_split_rng_state draws fresh
 * coefficients (a host key in the kernel arguments would be frozen into the graph).  One state per stream of
 * launches; ffgpu_rng_state_init is not capturable (it synchronises).  mul_by: NULL or the second factor of
 * the fused local product (as ffgpu_mul_split_rng).  No reference counterpart (secrets.randbelow, thresha.py:58). */
size_t ffgpu_rng_state_bytes(void);
int ffgpu_rng_state_init(ffgpu_ctx* ctx, void* dev_state, const uint8_t* host_key32, uint64_t nonce, int rounds,
                         void* stream);
int ffgpu_split_rng_state(ffgpu_ctx* ctx, const void* secrets, const void* mul_by, void* dev_state, int t, int m,
                          void* shares, size_t share_stride, size_t n, void* stream);

/* ---- Lagrange recombination ------------------------------------------- */
/* out[r][h] = sum_{j<k} lambda[r][j] * rows[j][h]  (mod modulus), r < w.
 * host_rows: HOST array of k device pointers (rows arrive from k peers and need
 * not be contiguous).  host_lambda: HOST array (w, k) of canonical scalars,
 * 2 x uint64 limbs each (from _recombination_vector, thresha.py:67-85, computed
 * on the host and cached there).  out is (w, n) with row stride out_stride.
 * Products are accumulated unreduced and reduced once, as the reference's
 * object matmul does (finfields.py:1126-1135).
 * replaces: thresha.py:119-132 np_recombine, thresha.py:88-116 recombine.     */
int ffgpu_recombine(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda,
                    int k, int w, void* out, size_t out_stride, size_t n, void* stream);

/* ---- dense matrix product ---------------------------------------------- */
/* C (M x N) = A (M x K) @ B (K x N) over the field, row-major with leading dimensions lda/ldb/ldc in
 * ELEMENTS; C must not overlap A or B.  The result is that of the reference's object matmul followed by one `%`
 * (exact integer accumulation, reduced at the end).  Kernel families, chosen by shape and field: one output dimension <= 8 ->
 * matrix x few columns / few rows x matrix kernels that read the big operand once (one-word primes: six multiply-adds per
 * term into column sums); prime fields with more than 8 rows and columns, K >= 64 and M*N*K >= 8e7 -> exact signed-digit
 * GEMMs on the int8 matrix cores (tiles padded to 64); otherwise an LDS-tiled vector-ALU kernel (split over K when
 * the output has few tiles).  The matrix-core and split-K paths keep digit planes / partial sums in grow-only
 * scratch buffers owned by the context, ONE PER STREAM (launches on different streams never share scratch): the
 * first call of a larger shape on a stream allocates its buffer (and synchronises that stream), so issue one such
 * call before capturing launches in a HIP graph.
 * replaces: finfields.py:1126-1146 (__matmul__: object matmul then one `%`), the local product of
 * runtime.py:2481-2541 np_matmul (A @ B at :2531).                                             */
int ffgpu_matmul(ffgpu_ctx* ctx, const void* A, size_t lda, const void* B, size_t ldb, void* C, size_t ldc,
                 size_t M, size_t K, size_t N, void* stream);

/* ---- stacks of matrix products ------------------------------------------------------ */
/* C[b] (M x N) = A[b] (M x K) @ B[b] (K x N) for b < batch, matrix b of an operand at element offset b * stride (row-major,
 * leading dimensions as for ffgpu_matmul).  stride_a == 0 or stride_b == 0: the one matrix is shared by the whole stack (no
 * expanded copy is needed).  Every matrix of the result is bit-identical to ffgpu_matmul on that pair.  Small and medium
 * matrices are ONE launch whatever the batch and need no scratch: M*N <= 256 -> several consecutive matrices per workgroup,
 * staged in LDS with coalesced loads, one output per thread; otherwise the LDS-tiled vector-ALU kernel with the matrix
 * index folded into the grid.  Matrices that ffgpu_matmul would give to the matrix cores, or with M*N*K at or above
 * FFGPU_MM_STACK_LOOP_MIN, run through ffgpu_matmul's routes one after the other inside
 * this call (same scratch rules).
 * batch == 0, M == 0 or N == 0: FFGPU_OK, nothing is touched; K == 0: zeros, as ffgpu_matmul.  FFGPU_EINVAL, nothing
 * launched: a leading dimension that is too short; a non-zero stride smaller than a matrix ((rows - 1) * ld + columns
 * elements); stride_c smaller than a matrix (zero only with batch == 1); sizes whose byte ranges overflow; more
 * workgroups than a grid holds; a C range that overlaps the A or B range.
 * replaces: finfields.py:1126-1135 (__matmul__ on stacks: NumPy's object matmul with broadcasting, then one `%`), the
 * local product of runtime.py:2481-2541 np_matmul "with broadcast" (A @ B at :2531).              */
int ffgpu_matmul_stack(ffgpu_ctx* ctx, const void* A, size_t lda, size_t stride_a, const void* B, size_t ldb, size_t stride_b,
                       void* C, size_t ldc, size_t stride_c, size_t M, size_t K, size_t N, size_t batch, void* stream);

/* ---- convolution ---------------------------------------------------------------- */
/* out[k] = sum_j a[k - j] * v[j] over the field, 0 <= k < na + nv - 1: the FULL convolution of two arrays
 * (np.convolve modes 'same' and 'valid' are slices of it, taken by the caller).  The operand order does not
 * matter: the shorter one becomes the tap vector.  One kernel, output-stationary tiles with the window of `a`
 * and the taps staged in LDS and the field's lazily reduced multiply-accumulate; it reads a and v, writes out
 * and uses no scratch memory, so memory is linear in na + nv.  na == 0, nv == 0 or an `out` that overlaps an
 * operand: FFGPU_EINVAL.
 * replaces: finfields.py:796-801 (np.convolve on the object arrays, then `%`), the local convolution of
 * runtime.py:2580-2627 np_convolve (np.convolve(a, b) at :2627).                                 */
int ffgpu_convolve(ffgpu_ctx* ctx, const void* a, size_t na, const void* v, size_t nv, void* out, void* stream);

/* ---- prefix scans and reductions along one axis ------------------------------------ */
/* The array is contiguous row-major (outer, k, inner): element (o, j, i) at (o*k + j)*inner + i.  That covers every axis
 * of every contiguous array without a transposed copy.  op: FFGPU_SCAN_ADD (field addition) or FFGPU_SCAN_MUL (field
 * multiplication); both are exact and associative, so the result does not depend on the order of evaluation.
 *
 * ffgpu_scan: out(o, j, i) = a(o, 0, i) op ... op a(o, j, i), the inclusive scan along j.  with_initial != 0: out has
 * k + 1 entries along the axis, the identity (0 / 1) first (np.cumulative_sum(include_initial=True)).  out == a (in
 * place) is allowed when with_initial == 0; any other overlap of out with a: FFGPU_EINVAL.
 * ffgpu_axis_reduce: out(o, i) = a(o, 0, i) op ... op a(o, k-1, i), outer*inner elements; out must not overlap a.
 * Two geometries (csrc/scan_geom.hpp): a column walk (one thread per column pack, running value in registers, one
 * launch, every element read once) when outer*inner fills the device, and row tiles otherwise (a workgroup scans a
 * tile; lines of several tiles take reduce-then-scan: tile aggregates, one scan of the aggregates, a second pass with the
 * carries -- three launches whatever k, and no workgroup ever waits for another).
 * workspace: ffgpu_scan_workspace_bytes(ctx, outer, k, inner) bytes of device memory, 16-byte aligned (tile aggregates
 * only: with the default tile one element per 4096 input elements, 2048 above 8-byte elements -- the query follows
 * FFGPU_SCAN_TILE_THREADS, which tests lower; may be NULL when the query returns 0).  A smaller one: FFGPU_EINVAL.
 * k == 0, outer*inner == 0, sizes whose product overflows size_t, or more tiles than a grid holds: FFGPU_EINVAL (the
 * query returns 0 for them); nothing is launched.
 * replaces: finfields.py:801, 807 (np.cumsum / np.cumprod on the object arrays, then `%`), finfields.py:1332-1349
 * (FiniteFieldArray.sum / .prod along an axis), runtime.py:3476-3506 np_sum with an axis, runtime.py:3510-3549
 * np_cumsum / np_cumulative_sum, the cumsum of runtime.py:3668 np_sgn.                                    */
#define FFGPU_SCAN_ADD 0
#define FFGPU_SCAN_MUL 1
int ffgpu_scan(ffgpu_ctx* ctx, int op, const void* a, void* out, size_t outer, size_t k, size_t inner, int with_initial,
               void* workspace, size_t workspace_bytes, void* stream);
int ffgpu_axis_reduce(ffgpu_ctx* ctx, int op, const void* a, void* out, size_t outer, size_t k, size_t inner,
                      void* workspace, size_t workspace_bytes, void* stream);
size_t ffgpu_scan_workspace_bytes(ffgpu_ctx* ctx, size_t outer, size_t k, size_t inner);

/* ---- secure comparison: the local steps of np_sgn ----------------------------------- */
/* What one party computes between the openings of runtime.np_sgn (a < 0, a == 0, sign), on its own shares.  Prime fields
 * only (FFGPU_ENOTSUP for GF(2^n)), integers (frac_length 0).  n values of bit length l; everything is mod p; bit index i
 * runs most significant first, as shifts = arange(l-1, -1, -1) does.  Shares are arbitrary canonical field elements:
 *   a[n]        the values;
 *   rbits[n*l]  element-major: rbits[h*l + i] is the share of the random bit of weight 2^(l-1-i) of element h;
 *   sbit[n]     the share of the sign-mask bit (the reference takes the last n random bits);
 *   rdivl[n]    the share of the high mask.
 * ffgpu_sgn_mask:   masked[h] = a[h] + 2^l + sum_i rbits[h*l+i] 2^(l-1-i) + rdivl[h] 2^l -- the value that is opened.
 *   replaces: runtime.py:3649-3657 (reshape, `r_bits << shifts`, the row sum, a_r, `a_r + (r_divl << l)`).
 * ffgpu_sgn_expand: c[n] is the opened public value (canonical).  With cl = c[h] mod 2^l (the canonical integer),
 *   cb_i = bit l-1-i of cl, r_i = rbits[h*l+i], s = 2 sbit[h] - 1, x_i = cb_i ? 1 - r_i : r_i, S_i = x_0 + ... + x_(i-1):
 *     e_out[i*n+h]  = s - cb_i + r_i + 3 S_i for i < l, e_out[l*n+h] = s - 1 + 3 S_l      bit-major (l+1, n)
 *     nx_out[i*n+h] = 1 - x_i                                                             bit-major (l, n)
 *     z_out[h]      = cl - a[h] - 2^l - sum_i r_i 2^(l-1-i)
 *   Each of e_out, nx_out, z_out may be NULL (all three: FFGPU_EINVAL); sbit may be NULL only when e_out is (the
 *   equality test draws no sign bit).  One kernel: a workgroup stages a tile of rbits through LDS with coalesced loads
 *   and every thread walks the bits of its own element, so the transposed outputs are written coalesced too
 *   (csrc/sgn_geom.hpp).
 *   replaces: runtime.py:3658-3671 (`c & mask`, z, right_shift.outer, the transpose, Xor, vstack, cumsum, e) and the
 *   `1 - Xor` of :3679 -- and the host-built c_bits with its upload.
 * ffgpu_sgn_finish: w[n] is the opened masked product of the rows of e; with g = (w[h] == 0):
 *     lt_out[h] = (z[h] + ((1 - 2g) s + 3) 2^(l-1)) 2^-l        -- the share of [a < 0].
 *   replaces: runtime.py:3674-3676 (g from the opened value, h, `Zp.array(z + (h << l-1)) >> l`).
 * All three are asynchronous on `stream`, allocate nothing and never synchronise (they can be captured in a HIP graph);
 * inputs are never written, outputs are canonical.  n == 0: FFGPU_OK.  FFGPU_EINVAL, nothing launched: a null context or
 * required pointer; l < 1, l > 64 or l > bit_length(p) - 2 (2^l, 2^(l-1) and 2^-l must be field elements); n*l or its
 * byte size overflowing; an output range that overlaps an input or another output.                              */
int ffgpu_sgn_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivl, int l, void* masked, size_t n,
                   void* stream);
int ffgpu_sgn_expand(ffgpu_ctx* ctx, const void* c, const void* a, const void* rbits, const void* sbit, int l, void* e_out,
                     void* nx_out, void* z_out, size_t n, void* stream);
int ffgpu_sgn_finish(ffgpu_ctx* ctx, const void* w, const void* sbit, const void* z, int l, void* lt_out, size_t n,
                     void* stream);

/* ---- sorting network: the two ends of a compare-exchange stage ------------------------ */
/* runtime.np_sort is Batcher's merge-exchange network along one axis.  The array is contiguous row-major (outer, k, inner),
 * element (o, j, i) at (o*k + j)*inner + i, the network runs along k (the convention of ffgpu_scan).  A stage is (p, d, r)
 * from the reference's loop: p a power of two and either r == 0, d == p, or r == p with d + p a larger power of two.  Its
 * index set I = { i < k - d : i & p == r } has P = ffgpu_cx_pairs(k, p, d, r) members, the j-th is
 * I_j = (j / p) * 2p + (j % p) + r, and I and I + d are disjoint (csrc/sort_geom.hpp).  Prime fields only (FFGPU_ENOTSUP
 * for GF(2^n)); everything is mod p.
 * ffgpu_cx_pairs: P; 0 for an invalid stage.  Needs no context and no device.
 * ffgpu_cx_diff:  out[(o*P + j)*inner + i] = a[o, I_j + d, i] - a[o, I_j, i] -- compact (outer, P, inner), the values
 *   the caller compares with zero.
 *   replaces: runtime.py:1764-1767 (the index array I, the gathers a[..., I] and a[..., I + d], b1 - b0).
 * ffgpu_cx_apply: with h = sum_s lambda[s] * rows[s][(o*P + j)*inner + i]:  a[o, I_j, i] += h and a[o, I_j + d, i] -= h,
 *   in place.  rows / lambda as for ffgpu_recombine (w = 1): the nrows sub-share rows of the re-shared product
 *   [b1 < b0] * (b1 - b0) a party received and the Lagrange vector, recombined in registers on the way; nrows = 1 with
 *   lambda = [1] applies an h that already exists.  1 <= nrows <= 9; more rows: FFGPU_ENOTSUP, the status
 *   ffgpu_recombine gives for more rows than it takes.  Positions of `a` outside I and I + d are not touched.
 *   replaces: runtime.py:1768-1770 (b0 + h, b1 - h, the two np_update scatters) and the recombination of the product
 *   before them (thresha.py:119-132).
 * Both are asynchronous on `stream`, allocate nothing and never synchronise (they can be captured in a HIP graph); inputs
 * are never written, outputs are canonical.  FFGPU_OK, nothing launched: outer*inner == 0 or P == 0.  FFGPU_EINVAL,
 * nothing launched: a null context or pointer; k < 2; (p, d, r) not a stage; nrows < 1; outer*k*inner or its byte size
 * overflowing; `out` or a row overlapping `a`.                                                                  */
size_t ffgpu_cx_pairs(size_t k, size_t p, size_t d, size_t r);
int ffgpu_cx_diff(ffgpu_ctx* ctx, const void* a, void* out, size_t outer, size_t k, size_t inner, size_t p, size_t d, size_t r,
                  void* stream);
int ffgpu_cx_apply(ffgpu_ctx* ctx, void* a, const void* const* host_rows, const uint64_t* host_lambda, int nrows, size_t outer,
                   size_t k, size_t inner, size_t p, size_t d, size_t r, void* stream);

/* ---- bit decomposition over a prime field: the local steps of np_to_bits -------------- */
/* What one party computes between the messages of runtime.np_to_bits over a prime field, on its own shares: the masked value
 * that is opened, and the addition of the opening's public bits to the shared random bits by the prefix-carry network of
 * runtime.np_add_bits.  Prime fields only (FFGPU_ENOTSUP for GF(2^n), which have ffgpu_gf256_to_bits), integers
 * (frac_length 0).  n values of l bits, 1 <= l <= 64 and l <= bit_length(p) - 2; everything is mod p; bit index k runs
 * LEAST significant first, as shifts = arange(l) does (the opposite of ffgpu_sgn_*).  Shares are arbitrary canonical field
 * elements:
 *   a[n]         the values;             rdivl[n]   the share of the high mask;
 *   rbits[n*l]   element-major: rbits[h*l + k] is the share of the random bit of weight 2^k of element h;
 *   g, p [l*n]   bit-major generate / propagate (carry) values: row k is the n contiguous elements at k*n.
 * The network (csrc/bits_geom.hpp): the reference's recursion f(i, j, high) splits [i, j) at h = i + (j-i)/2 and merges with
 * c2 += c1[-1] * d2 and, when high (i > 0), d2 *= d1[-1].  A merge runs in round ceil(log2(j - i)); round rho = 1 ..
 * ffgpu_carry_rounds(l) = ceil(log2 l) is a list of Rc c-products g[q]*p[k] for every k of the right half of every merge
 * of the round, q = h - 1, k ascending, then Rd d-products p[q]*p[k] for the same (k, q) of the merges with i > 0, k
 * ascending; R = Rc + Rd <= 63.  Within a round the k are distinct, no q is among them, and every product reads values
 * from before the round.
 * ffgpu_carry_rounds: the number of rounds (0 for l == 1); -1 unless 1 <= l <= 64.
 * ffgpu_carry_rows:   *rc = Rc, *rd = Rd of the round.
 * ffgpu_carry_level:  k_out[j], q_out[j] for the R product rows of the round, the c-products first (room for 63 each).
 *   These three are host functions: no context, no device.  FFGPU_EINVAL: l or round out of range, a null pointer.
 * ffgpu_bits_mask:   masked[h] = a[h] + offset + rdivl[h] 2^l - sum_k rbits[h*l+k] 2^k -- the value that is opened.
 *   host_offset: one canonical host scalar (ffgpu_ctx_scalar_limbs words); the reference uses 2^bit_length.
 *   replaces: runtime.py:4414-4415 (`r_bits << shifts`, the row sum) and :4446 (a + offset + (r_divl << l) - r_modl).
 * ffgpu_bits_expand: c[n] is the opened public value (canonical).  With cb_k = bit k of the canonical integer
 *   c[h] mod 2^l and r = rbits[h*l+k]:  g_out[k*n+h] = cb_k ? r : 0,  p_out[k*n+h] = cb_k ? 1 - r : r  -- the leaves
 *   a_i*b_i and a_i + b_i - 2 a_i b_i of the network for a public b.  One kernel: a workgroup stages a tile of rbits
 *   through LDS with coalesced loads (the tiles and chunks of csrc/sgn_geom.hpp) and every thread walks the bits of its own
 *   element, so both bit-major outputs are written coalesced.
 *   replaces: runtime.py:4447-4448 (`(c >> shifts) & 1`, np_add_bits), the leaf case of :4309-4314, and the host-built
 *   c_bits with its upload.
 * ffgpu_carry_prod:  out[j*n+h] = g[q_j*n+h] * p[k_j*n+h] for j < Rc, out[(Rc+j)*n+h] = p[q_j*n+h] * p[k_j*n+h] for the
 *   d-products: compact (R, n), the party's local degree-2t products of the round.  Every operand element is read once per
 *   product row; nothing else is read or written.
 *   replaces: the gathers and `c1[-1] * d2`, `d2 * d1[-1]` of runtime.py:4320-4325 (the local part of np_multiply).
 * ffgpu_carry_apply: with v = sum_s lambda[s] * rows[s][j*n+h] recombined in registers:  g[k_j*n+h] += v for the c-rows,
 *   p[k_j*n+h] = v for the d-rows, in place.  rows / lambda as for ffgpu_cx_apply: the nrows sub-share rows of the re-shared
 *   products a party received and the Lagrange vector; 1 <= nrows <= 9, more rows: FFGPU_ENOTSUP.  Rows of g and p
 *   outside the round's k are not touched.
 *   replaces: runtime.py:4320-4325 (c2 + ..., the new d2, the concatenations) and the recombination of _reshare before
 *   it (thresha.py:119-132).
 * ffgpu_bits_finish: out[h*l+k] = rbits[h*l+k] + cb_k - 2 g[k*n+h] + (k > 0 ? g[(k-1)*n+h] : 0), element-major, g the
 *   prefix carries after the last round.  The loads of rbits and the stores of out both go through the LDS tile, so both
 *   element-major sides are coalesced.
 *   replaces: runtime.py:4332-4334 (the shifted carries, a + b - 2c + c_shifted) with the transposes around it.
 * The five device entries are asynchronous on `stream`, allocate nothing and never synchronise (the round's table travels in
 * the kernel arguments: they can be captured in a HIP graph); inputs are never written, outputs are canonical.  FFGPU_OK,
 * nothing launched: n == 0, or a round without product rows.  FFGPU_EINVAL, nothing launched: a null context or required
 * pointer; l < 1, l > 64 or l > bit_length(p) - 2; round < 1 or round > ffgpu_carry_rounds(l); nrows < 1; n*l or its byte
 * size overflowing; an output range that overlaps an input or another output, g overlapping p, a row overlapping g or p. */
int ffgpu_carry_rounds(int l);
int ffgpu_carry_rows(int l, int round, int* rc, int* rd);
int ffgpu_carry_level(int l, int round, uint8_t* k_out, uint8_t* q_out);
int ffgpu_bits_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivl, const uint64_t* host_offset, int l,
                    void* masked, size_t n, void* stream);
int ffgpu_bits_expand(ffgpu_ctx* ctx, const void* c, const void* rbits, int l, void* g_out, void* p_out, size_t n, void* stream);
int ffgpu_carry_prod(ffgpu_ctx* ctx, const void* g, const void* p, int l, int round, void* out, size_t n, void* stream);
int ffgpu_carry_apply(ffgpu_ctx* ctx, void* g, void* p, const void* const* host_rows, const uint64_t* host_lambda, int nrows,
                      int l, int round, size_t n, void* stream);
int ffgpu_bits_finish(ffgpu_ctx* ctx, const void* c, const void* rbits, const void* g, int l, void* out, size_t n, void* stream);

/* ---- tournament along an axis: the ends of a round ------------------------------------ */
/* runtime.np_amax / np_amin and runtime.np_argmax / np_argmin halve an axis per round: pairs are compared, the winner of a
 * pair survives.  The array is contiguous row-major (outer, k, inner), element (o, j, i) at (o*k + j)*inner + i, the round
 * runs along k >= 2 (the convention of ffgpu_scan).  n0 = k % 2, h = k / 2 pairs, kc = h + n0 survivors; position 0 is the
 * bye when n0.  Pair j < h is (first_j, second_j) (csrc/tour_geom.hpp):
 *   FFGPU_TOUR_HALVES    (n0 + j, kc + j)           np_amax / np_amin, runtime.py:3415, 3464
 *   FFGPU_TOUR_ODD_EVEN  (n0 + 2j, n0 + 2j + 1)     _np_argmax / _np_argmin, runtime.py:3807, 3935 (the first occurrence wins)
 * Prime fields only (FFGPU_ENOTSUP for GF(2^n)), integers (frac_length 0); everything is mod p.
 * ffgpu_tour_diff: out[(o*h + j)*inner + i] = a[o, second_j, i] - a[o, first_j, i] for neg = 0 (the minimum: the value
 *   compared with zero is a2 - a1), a[o, first_j, i] - a[o, second_j, i] for neg = 1 (the maximum: c = [a1 < a2]) --
 *   compact (outer, h, inner).
 *   replaces: runtime.py:3415-3416, 3464-3465, 3807-3808, 3935-3936 (the two slices and their difference).
 * ffgpu_tour_select: with v = sum_s lambda[s] * rows[s][(o*h + j)*inner + i]:  out[o, n0 + j, i] = a[o, first_j, i] + v for
 *   neg = 0, - v for neg = 1, and out[o, 0, i] = a[o, 0, i] when n0; out is the next level (outer, kc, inner), not written
 *   in place.  rows / lambda as for ffgpu_cx_apply: the nrows sub-share rows of the re-shared product c * (difference) a
 *   party received and the Lagrange vector, recombined in registers on the way; nrows = 1 with lambda = [1] applies a v
 *   that already exists.  1 <= nrows <= 9; more rows: FFGPU_ENOTSUP.
 *   replaces: runtime.py:3416-3418, 3465-3467, 3810-3812, 3938-3940 (a1 + product, the concatenation with the bye) and the
 *   recombination of the product before them (thresha.py:119-132).
 * ffgpu_tour_unit_prod: out[(o*h + j)*inner + i] = u[o, n0 + j, i] * c[(o*h + j)*inner + i] -- compact; u is (outer, kc,
 *   inner), the child level's unit vectors, c this level's kept comparison bits: the party's local degree-2t product of the
 *   upward pass.
 *   replaces: runtime.py:3815-3816, 3943-3944 (u[:, 1:] and the local part of u * c).
 * ffgpu_tour_unit_expand: v as for ffgpu_tour_select:  out[o, n0 + 2j, i] = u[o, n0 + j, i] - v, out[o, n0 + 2j + 1, i] = v,
 *   and out[o, 0, i] = u[o, 0, i] when n0; out is (outer, k, inner).  1 <= nrows <= 9 as above; rows = [c], lambda = [1] is
 *   the round whose child has length 1 (runtime.py:3803, 3931).
 *   replaces: runtime.py:3817-3820, 3945-3948 (u - u2, the concatenation, the order='F' reshape, u0 re-attached) and the
 *   recombination of u * c before them.
 * All four are asynchronous on `stream`, allocate nothing and never synchronise (they can be captured in a HIP graph);
 * inputs are never written, outputs are canonical.  FFGPU_OK, nothing launched: outer*inner == 0.  FFGPU_EINVAL, nothing
 * launched: a null context or pointer; k < 2; an unknown mode; nrows < 1; outer*k*inner or its byte size overflowing; an
 * output overlapping an input or a row.                                                                           */
#define FFGPU_TOUR_HALVES   0
#define FFGPU_TOUR_ODD_EVEN 1
int ffgpu_tour_diff(ffgpu_ctx* ctx, const void* a, void* out, size_t outer, size_t k, size_t inner, int mode, int neg,
                    void* stream);
int ffgpu_tour_select(ffgpu_ctx* ctx, const void* a, const void* const* host_rows, const uint64_t* host_lambda, int nrows,
                      void* out, size_t outer, size_t k, size_t inner, int mode, int neg, void* stream);
int ffgpu_tour_unit_prod(ffgpu_ctx* ctx, const void* u, const void* c, void* out, size_t outer, size_t k, size_t inner,
                         void* stream);
int ffgpu_tour_unit_expand(ffgpu_ctx* ctx, const void* u, const void* const* host_rows, const uint64_t* host_lambda, int nrows,
                           void* out, size_t outer, size_t k, size_t inner, void* stream);

/* ---- first occurrence along an axis: the ends of a round ------------------------------ */
/* runtime.np_find (runtime.py:4603-4698) returns the index, or a function f of the index, of the first 0 along an axis of
 * an array of shared bits (after its reduction of "first s" to "first 0").  A node of its tree is the stack (nf, v_1 .. v_F):
 * nf = 1 for "no 0 in my interval", v_q the running value of the conditional-step function cs_f; two neighbouring intervals
 * combine as L + nf_L * (R - L) (np_where(nf[0], R, L), runtime.py:4684).  The combine is associative and keeps order, so
 * the rounds here pair neighbours as FFGPU_TOUR_ODD_EVEN does: over kk positions n0 = kk % 2, h = kk / 2 pairs
 * (first_j, second_j) = (n0 + 2j, n0 + 2j + 1), kc = h + n0 survivors, position 0 the bye when n0 (csrc/find_geom.hpp).
 * Prime fields only (FFGPU_ENOTSUP for GF(2^n)), integers (frac_length 0); everything is mod p.
 *   bits   contiguous row-major (outer, k, inner), k >= 1: one party's shares of values in {0, 1}; the search runs along k.
 *   level  component-major (C, outer, kk, inner), C = ncomp = 1 + F components, 1 <= F <= 4; component 0 is nf.
 *   virt   0 or 1; the leaf round runs over kv = k + virt positions.  With virt, position k is the public leaf (1, f(e)):
 *          the value for "not found" enters as a leaf, so the root's v is the answer and the reference's last gate
 *          (np_where(nf, f(e), f_ix), runtime.py:4692) is not needed.  Position k is the second member of the last pair and
 *          has no memory behind it.
 *   tab    device array (F, 2, kv) of canonical elements: tab[q, 0, j] = cs_f(0, j)_q, tab[q, 1, j] = cs_f(1, j)_q -
 *          cs_f(0, j)_q, and with virt tab[q, 0, k] = f(e)_q, tab[q, 1, k] = 0.
 *   leaf j = (b', tab[q, 0, j] + b' * tab[q, 1, j]) with b' = bits[o, j, i] for flip = 0 and 1 - bits[o, j, i] for flip = 1
 *          (the reference's public s = 1, runtime.py:4631-4632); the public leaf has b' = 1 and is not flipped.  leaf_0 is
 *          b', leaf_q for q >= 1 the value component q.  The leaf level is never stored.
 * ffgpu_find_leaf_prod: out[q, o, j, i] = leaf_0(first_j) * (leaf_q(second_j) - leaf_q(first_j)) -- compact (C, outer, h,
 *   inner) over the kv positions: the party's local degree-2t product of the first round.
 *   replaces: runtime.py:4679-4680 (the leaves and their stack) and the local part of the first np_where (:4684).
 * ffgpu_find_leaf_apply: with v = sum_s lambda[s] * rows[s][q, o, j, i]:  out[q, o, n0 + j, i] = leaf_q(first_j) + v, and
 *   out[q, o, 0, i] = leaf_q(0) when n0; out is the next level (C, outer, kc, inner).  rows / lambda as for
 *   ffgpu_tour_select: the nrows compact (C, outer, h, inner) sub-share rows of the re-shared product and the Lagrange
 *   vector, recombined in registers on the way; nrows = 1 with lambda = [1] applies a v that already exists.
 *   replaces: the rest of the first np_where (runtime.py:4684) and the recombination before it (thresha.py:119-132).
 * ffgpu_find_prod: for a stored level (C, outer, k, inner), k >= 2:  out[q, o, j, i] = level[0, o, first_j, i] *
 *   (level[q, o, second_j, i] - level[q, o, first_j, i]) -- compact (C, outer, h, inner).
 *   replaces: the local part of np_where(nf[0], cl(h, j), nf) of the inner nodes (runtime.py:4683-4684).
 * The apply of a later round is ffgpu_tour_select on (C * outer, k, inner) with FFGPU_TOUR_ODD_EVEN and neg = 0: the
 * components are more rows of the same round.
 * All three are asynchronous on `stream`, allocate nothing and never synchronise (they can be captured in a HIP graph);
 * inputs are never written, outputs are canonical.  In every case below nothing is written and nothing is launched.
 * FFGPU_OK: outer*inner == 0.  FFGPU_EINVAL: a null context or pointer; k < 1 (k < 2 for ffgpu_find_prod); kv < 2 for the
 * leaf calls; ncomp outside 2..5 (this one rule covers more than four value components too); flip or virt outside {0, 1};
 * ncomp*outer*kv*inner or its byte size overflowing; an output overlapping the bits, the level, a row or the table.
 * FFGPU_ENOTSUP: a GF(2^n) context; nrows outside 1..9.                                                            */
int ffgpu_find_leaf_prod(ffgpu_ctx* ctx, const void* bits, const void* tab, void* out, size_t outer, size_t k, size_t inner,
                         int ncomp, int flip, int virt, void* stream);
int ffgpu_find_leaf_apply(ffgpu_ctx* ctx, const void* bits, const void* tab, const void* const* host_rows,
                          const uint64_t* host_lambda, int nrows, void* out, size_t outer, size_t k, size_t inner, int ncomp,
                          int flip, int virt, void* stream);
int ffgpu_find_prod(ffgpu_ctx* ctx, const void* level, void* out, size_t outer, size_t k, size_t inner, int ncomp, void* stream);

/* ---- fixed point: truncation and the gate of the normalisation ------------------------ */
/* A fixed-point number with f fractional bits and bit length l is the field element a = round(x * 2^f), -2^(l-1) <= a <
 * 2^(l-1); everything below is on these raw integers mod p.  runtime.np_trunc (runtime.py:839-873) divides by 2^f with
 * probabilistic rounding: it masks a with f random bits and a high mask, opens the sum, and subtracts the opened value's low
 * f bits again.  runtime._norm (runtime.py:4718-4727) decomposes a into bits, and searches the bits below the sign bit, most
 * significant first, for the first one that equals the SECRET inverted sign bit s = 1 - x_top; the gate s + (1 - 2s) x turns
 * that into the search for the first 0 that ffgpu_find_* serve.  Prime fields only (FFGPU_ENOTSUP for GF(2^n)).  Bit index
 * k runs LEAST significant first, as for ffgpu_bits_*.  Shares are arbitrary canonical field elements:
 *   a[n], rdivf[n], ar[n]   the values, the share of the high mask, a + the value of the random bits;
 *   rbits[n*f]   element-major: rbits[h*f + k] is the share of the random bit of weight 2^k of element h;
 *   bits[n*l]    what ffgpu_bits_finish writes: element-major, so x_top = bits[h*l + l-1] is the share of the sign bit.
 * ffgpu_trunc_mask:  ar_out[h] = a[h] + sum_k rbits[h*f+k] 2^k;  masked_out[h] = ar_out[h] + offset + rdivf[h] 2^f -- the
 *   value that is opened.  host_offset: one canonical host scalar as for ffgpu_bits_mask; the reference uses 2^(l-1) with l
 *   the bit length of a.  Both outputs are required: ar is kept so that the finish reads one element per value, not f.  One
 *   kernel, built as the one of ffgpu_bits_mask (the tiles and chunks of csrc/sgn_geom.hpp).
 *   replaces: runtime.py:860-861 (`r_bits << arange(f)`, the row sum) and :869-870 (ar_modf += a, + 2^(l-1) + (r_divf << f)).
 * ffgpu_trunc_finish: with c = sum_s lambda[s] * rows[s][h] recombined in registers and taken as its canonical integer:
 *   out[h] = (ar[h] - (c mod 2^f)) * 2^-f.  rows / lambda as for ffgpu_tour_select: the nrows masked shares a party received
 *   (t+1 of them) and the Lagrange vector, so the opened value never goes to memory; nrows = 1 with lambda = [1] takes a c
 *   that is already open.  1 <= nrows <= 9; more rows: FFGPU_ENOTSUP.
 *   replaces: the recombination inside output() (thresha.py:119-132) and runtime.py:871-872 (c & (2^f - 1), the shift).
 * ffgpu_norm_prod:   out[h*(l-1) + j] = (2 x_top - 1) * bits[h*l + l-2-j] for j < l-1 -- compact (n, l-1): the party's
 *   local degree-2t product of (1 - 2s) with the bits below the sign bit, reversed.  sign_out[h] = 1 - 2 x_top = 2s - 1
 *   (local, degree t); it may be NULL.
 *   replaces: runtime.py:4723-4725 (s, the slice, np.flip) and the local part of the gate at :4636.
 * ffgpu_norm_apply:  out[h*(l-1) + j] = 1 - x_top + sum_s lambda[s] * rows[s][h*(l-1) + j] -- s + (1 - 2s) x as a dense
 *   (outer = n, k = l-1, inner = 1) array: what ffgpu_find_leaf_prod / _apply search for its first 0.  rows: the nrows compact
 *   (n, l-1) sub-share rows of the re-shared product.  1 <= nrows <= 9; more rows: FFGPU_ENOTSUP.
 *   replaces: the rest of runtime.py:4636 and the recombination before it.
 * All four are asynchronous on `stream`, allocate nothing and never synchronise (they can be captured in a HIP graph);
 * inputs are never written, outputs are canonical.  In every case below nothing is written and nothing is launched.
 * FFGPU_OK: n == 0.  FFGPU_EINVAL: a null context or required pointer; f < 1, f > 64 or f > bit_length(p) - 2; l < 2 or
 * l > 64; nrows < 1; n*f, n*l or its byte size overflowing; an output overlapping an input, a row or another output.
 * FFGPU_ENOTSUP: a GF(2^n) context; nrows > 9.                                                                       */
int ffgpu_trunc_mask(ffgpu_ctx* ctx, const void* a, const void* rbits, const void* rdivf, const uint64_t* host_offset, int f,
                     void* ar_out, void* masked_out, size_t n, void* stream);
int ffgpu_trunc_finish(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int nrows, const void* ar, int f,
                       void* out, size_t n, void* stream);
int ffgpu_norm_prod(ffgpu_ctx* ctx, const void* bits, int l, void* out, void* sign_out, size_t n, void* stream);
int ffgpu_norm_apply(ffgpu_ctx* ctx, const void* bits, const void* const* host_rows, const uint64_t* host_lambda, int nrows, int l,
                     void* out, size_t n, void* stream);

/* ---- square roots, p = 1 (mod 4) --------------------------------------------- */
/* out[i] = the square root the reference returns for a[i] (Cipolla-Lehmer with the smallest b such that
 * b^2 - 4a is a non-residue; 0 for a = 0).  Primes p = 3 (mod 4) and GF(2^n) take ffgpu_pow with the
 * exponents (p+1)/4 resp. q/2; FFGPU_ENOTSUP for those here.
 * replaces: finfields.py:447-470 (PrimeFieldElement._sqrt) mapped over arrays by :1459-1460.          */
int ffgpu_sqrt_cl(ffgpu_ctx* ctx, const void* a, void* out, size_t n, void* stream);

/* ---- Gaussian elimination ---------------------------------------------------- */
/* In place on `batch` row-major (n x ncols) matrices stored back to back (ncols >= n).
 * mode 0 (solve): (A | B) -> (. | A^-1 B), Gauss-Jordan; the solution occupies columns n..ncols-1.
 * mode 1 (det):   forward elimination only; det_out[b] = product of the pivots chosen by the reference's
 *                 rule (first nonzero entry at or below the diagonal; finfields.py:933-947 -- NB the
 *                 reference does not negate on row swaps, and neither does this), 0 if singular.
 * dev_singular: `batch` ints in device memory, set to 1 for singular matrices (whose contents are then
 *               unspecified); the caller raises ZeroDivisionError('no inverse exists') (finfields.py:893).
 * Nothing but the matrices, the `batch` flags and, in mode 1, the `batch` elements of det_out is written; with
 * batch = 0 or n = 0 nothing is written at all.
 * replaces: finfields.py:872-908 gauss_solve, :910-916 gauss_inv, :918-955 gauss_det
 *           (np.linalg.solve / inv / det / matrix_power with negative exponent on field arrays).     */
int ffgpu_gauss(ffgpu_ctx* ctx, void* a, int n, int ncols, size_t batch, int mode, void* det_out,
                void* dev_singular, void* stream);

/* ---- small public matrix over the last axis --------------------------------- */
/* out[i*r + a] = bias[a] + sum_{c<g} M[a][c] * in[i*g + c]  for every group i of g consecutive elements
 * (r, g <= 16).  host_matrix: (r, g) canonical 2-limb scalars; host_bias: r scalars or NULL.
 * replaces: finfields.py:1126-1146 `A @ x[..., np.newaxis]` with a public A and trailing axis g
 * (demos/np_aes.py:40-41: the S-box's GF(2) affine map on the 8 bit-shares of every byte, `+ B`),
 * and runtime.py:4475-4484 np_from_bits (sum_j x_j * 2^j over the last axis: r = 1).               */
int ffgpu_group_matvec(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, int r, int g,
                       const void* in, void* out, size_t ngroups, void* stream);

/* ---- reductions ------------------------------------------------------------- */
/* out[0] = sum_i a[i]*b[i]  (ffgpu_dot)  /  sum_i a[i]  (ffgpu_sum), one field element.
 * workspace: device scratch of at least FFGPU_REDUCE_WORKSPACE_BYTES bytes (per concurrent call).  The library never
 *            writes more than that many bytes of it, whatever the element size (the number of partial sums is bounded by
 *            what the workspace holds), and writes none of it when n = 0; nothing else but out[0] is written.
 * replaces: the local part of runtime.py in_prod / np_sum-style reductions (sum(map(mul, x, y)) on
 * shares, then one reshare) and FiniteFieldArray reductions through __array_function__ (np.sum).    */
#define FFGPU_REDUCE_WORKSPACE_BYTES (1024 * 16)
int ffgpu_dot(ffgpu_ctx* ctx, const void* a, const void* b, void* out, void* workspace, size_t n, void* stream);
int ffgpu_sum(ffgpu_ctx* ctx, const void* a, void* out, void* workspace, size_t n, void* stream);

/* ---- pseudorandom secret sharing: combination step ----------------------- */
/* HOST function: out_i = SHAKE128(msg_i) squeezed to out_len bytes, for nstreams independent messages on up
 * to `threads` host threads (<= 0: all cores).  One sponge is sequential, so a stream cannot be spread over
 * GPU lanes; the C(m, t) subset keys of a PRSS call can be spread over host cores.  Outputs go to caller
 * buffers (pin them and upload them as the `host_streams` of ffgpu_prss_combine).
 * replaces: thresha.py:255 `shake_128(self.key + s).digest(n * self.byte_length)`, once per key.         */
/* 1 if ffgpu_shake128_expand squeezes through the system's libcrypto (loaded at run time, checked against the
 * SHAKE128("") known answer), 0 if through the portable Keccak-f[1600] of the library (also with FFGPU_SHAKE_OWN=1). */
int ffgpu_shake128_backend(void);
int ffgpu_shake128_expand(const uint8_t* const* msgs, const size_t* msg_lens, int nstreams, size_t out_len,
                          uint8_t* const* outs, int threads);
/* The same streams, RESUMABLE: open absorbs the nstreams messages (*handle owns the sponge states), every squeeze
 * call writes the NEXT nbytes of stream i to outs[i] (nstreams host pointers; up to `threads` host threads, <= 0: all
 * cores), close frees the handle.  This is how the mirror runs a large PRSS call: a slice of every stream is squeezed
 * into one half of a bounded pinned buffer while the previous slice uploads and ffgpu_prss_combine consumes it on the
 * device (measured on the MI355X box, m = 7, t = 3, 10^7 draws: profiles/r03_api_path.md).
 * replaces: the same line, thresha.py:255 (hashlib squeezes a stream in one piece).                                */
int ffgpu_shake128_open(const uint8_t* const* msgs, const size_t* msg_lens, int nstreams, void** handle);
int ffgpu_shake128_squeeze(void* handle, uint8_t* const* outs, size_t nbytes, int threads);
void ffgpu_shake128_close(void* handle);

/* out[h] (+)= sum_{s<ks} sum_{j<d} draw_s[h*d + j] * weights[s][j]   (mod modulus)
 * host_streams: HOST array of ks DEVICE pointers to the raw SHAKE128 output of subset s
 * (n*d*l bytes each; the XOF is sequential per key and is computed on the host with hashlib, as in
 * thresha.PRF.__call__, thresha.py:238-266).  draw = l-byte little-endian chunk reduced into
 * range(bound): mask_bits == 0 -> bound is the field order (wide reduction, l = byte_length + 16),
 * mask_bits = b > 0 -> bound = 2^b (runtime.py:4062-4076 rounds bounds to powers of two).
 * host_weights: (ks, d) canonical 2-limb scalars f_S(i) * (i+1)^power from _f_S_i (thresha.py:135-141).
 * Limits per call: ks <= 48 and ks * d <= 96 (FFGPU_ENOTSUP beyond them, as ffgpu_recombine answers for too many
 * rows: split the subsets over several calls, the later ones with accumulate != 0); ks >= 1, d >= 1, 1 <= l <= 64 bytes
 * per draw, 0 <= mask_bits <= 192 with 2^mask_bits <= order (a masked draw is used as the field element it is), and
 * non-null host_streams, host_streams[s], host_weights and out (FFGPU_EINVAL otherwise).  A refused call launches nothing
 * and writes nothing; n = 0 is FFGPU_OK and touches no pointer.
 * Memory: the streams and the weights are never written; nothing outside the n elements of `out` is written; `out` may
 * start at any multiple of the element size (no 16-byte alignment is needed); with accumulate != 0 every element of `out`
 * is read exactly once, before it is stored, and out[h] depends on no other element of `out`; the n results are canonical.
 * replaces: thresha.py:163-173 np_pseudorandom_share (d = 1), :201-217 np_pseudorandom_share_0,
 * and the list versions :144-160, :176-198.                                                    */
int ffgpu_prss_combine(ffgpu_ctx* ctx, const void* const* host_streams, int ks, int d, int l, int mask_bits,
                       const uint64_t* host_weights, int accumulate, void* out, size_t n, void* stream);

/* PRODUCTION mode of the same combination: the draws come from a COUNTER-MODE PRF expanded on the device instead of the
 * reference's SHAKE128 stream (a sponge is sequential per key: in parity mode the host squeezes and the device idles).
 * host_keys: ks x 40 bytes, per subset key the 32-byte ChaCha key followed by the 8-byte nonce, both derived by the caller
 * from (PRF key, common input) -- the mirror uses shake_128(b"mpyc_amd prss chacha v1\0" + len(key) + key + input).digest(40).
 * A draw is l little-endian KEYSTREAM bytes reduced into range(bound) by the reference's own rule (`% bound`,
 * l = byte_length + len(key), thresha.py:234-236, or a mask for bound = 2^mask_bits), so a draw depends on (key, input,
 * index, bound) only -- not on the field (runtime.py:758-761 evaluates one set of PRFs over two fields).  rounds: 20, 12 or 8.
 * Layout of the keystream: ffgpu_prss_chacha_layout (tb blocks per tile of dpt draws, ceil(l/4) words per draw; draw j of
 * element h sits in tile h / dpt, slot h % dpt, block counters (tile * d + j) * tb + b).  Every party must use the same
 * mode; there is no reference counterpart for the PRF itself (pinned to RFC 8439 and to oracle/fforacle.c
 * orc_prss_chacha, not to reference outputs), the combination is the reference's.  Limits per call: ks <= 32 and
 * ks * d <= 64 (FFGPU_ENOTSUP beyond them; the later calls of a split one accumulate); ks >= 1, d >= 1, 1 <= l <= 64 bytes
 * per draw (the mirror raises NotImplementedError for wider draws), rounds in {20, 12, 8}, 0 <= mask_bits <= 192 with
 * 2^mask_bits <= order, non-null host_keys, host_weights and out (FFGPU_EINVAL otherwise).  The memory contract is that of
 * ffgpu_prss_combine: nothing but the n elements of `out` is written, at any element alignment, each read once before it
 * is stored when accumulate != 0; results are canonical; a refused call writes nothing.
 * replaces: thresha.py:163-173, 201-217 (np_pseudorandom_share, np_pseudorandom_share_0) with PRF := ChaCha.      */
int ffgpu_prss_chacha(ffgpu_ctx* ctx, const uint8_t* host_keys, int ks, int d, int l, int mask_bits, int rounds,
                      const uint64_t* host_weights, int accumulate, void* out, size_t n, void* stream);
int ffgpu_prss_chacha_layout(int l, int* tb, int* dpt);

/* ---- GF(2^8) S-box layer (local / public values) ----------------------- */
/* GF(2^n<=8), the linear layer of the AES S-box on BIT SHARES: for every group of 8 elements (the shares of the
 * 8 bits of one byte, 8-byte aligned): y = M x + bias with a public 8x8 matrix M (row-major canonical scalars);
 * from_bits = 0: out = y (8 elements per group); from_bits = 1: out = sum_r 2^r y_r (one element per group).
 * replaces: demos/np_aes.py:40-42 (`A @ x[..., np.newaxis]`, `x += B`, `mpc.np_from_bits(x)`) in one pass;
 *           finfields.py:1126-1146 + runtime.py:4475-4484.  ffgpu_group_matvec is the general form.           */
int ffgpu_gf256_bit_affine(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, int from_bits,
                           const void* in, void* out, size_t n, void* stream);

/* GF(2^n<=8): out[8 i + j] = ((in[i] >> j) & 1) + addend[8 i + j] for PUBLIC bytes `in` (addend may be NULL):
 * the local tail of the secure bit decomposition over a binary field, where every party adds the bits of the
 * opened masked value c to its shares of the random bits.
 * replaces: runtime.py:4418-4423 (`c_bits = np.int8(np.right_shift.outer(c, shifts) & 1); return c_bits + r_bits`). */
int ffgpu_gf256_to_bits(ffgpu_ctx* ctx, const void* in, const void* addend, void* out, size_t n, void* stream);

/* The secure bit decomposition of runtime.np_to_bits over GF(2^8) (runtime.py:4411-4423) with the two local steps
 * around its opening fused, for a computation whose parties all live on this GPU (mpyc_amd/protocols.py):
 *
 * ffgpu_gf256_mask_open: out[h] = sum_r coef[r] * rows[r][h] + sum_p mu[p] * (sum_b 2^b rbits_p[8h + b])
 *   = the opened masked value c = a + r_modl (runtime.py:4414-4421: `r_modl` by Horner over the bit shares, `a + r_modl`,
 *   `output`) computed straight from the t+1 opening parties' shares: rows/coef = their shares of a, each possibly
 *   still a pending recombination of sub-share rows (coef = mu_p * lambda_s, <= 32 rows), rbits_p = their shares of the
 *   random bits (8 per byte, 16-byte aligned, <= 8 parties).  One pass instead of 3 per party + 1.
 * ffgpu_gf256_bits_affine_fold: out_y[h] = sum_r 2^r (M (bits(c[h]) + rbits_y[8h..8h+7]) + bias)_r for parties
 *   y < nbatch (rbits_y = rbits + y*rbits_batch_stride, out_y = out + y*out_batch_stride; one launch, grid rows = y)
 *   = `c_bits + r_bits` (runtime.py:4422-4423), the public affine map over the bit shares and np_from_bits
 *   (demos/np_aes.py:40-42, runtime.py:4475-4484) without the 8n-byte bit arrays ever reaching HBM.                */
int ffgpu_gf256_mask_open(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_coef, int nrows,
                          const void* const* host_rbits, const uint64_t* host_mu, int np, void* out, size_t n, void* stream);
int ffgpu_gf256_bits_affine_fold(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, const void* c,
                                 const void* rbits, size_t rbits_batch_stride, void* out, size_t out_batch_stride, size_t n,
                                 int nbatch, void* stream);

/* The WHOLE secure AES S-box layer (demos/np_aes.py:37-43) for all m parties of a computation held on one GPU, in ONE
 * launch: x^254 by the reference's addition chain (11 secure multiplications: local products of the 2t+1 senders,
 * re-sharing with coefficients from the device CSPRNG, recombination with host_lambda = the Lagrange vector of the
 * senders 1..2t+1 at 0; runtime.py:1356-1367, 1096-1141, 603-689), np_to_bits (opening of y + r_modl from parties
 * 1..t+1 with host_mu, bits + r_bits; runtime.py:4411-4423), the GF(2) affine map host_matrix / host_bias on the bit
 * shares and np_from_bits.  Everything is element-wise, so a thread carries the m shares of four bytes through the
 * whole protocol in registers: 10 m bytes of HBM traffic per secure byte instead of the 269 of the per-step kernels.
 * x / out: m rows of n bytes (row strides in bytes, multiples of 4); rbits: m rows of 8 n bit shares (stride a
 * multiple of 16).  GF(2^8) only; any n (the n % 4 bytes after the last whole word of each row are handled with byte
 * accesses), every (m, t) with 2t+1 <= m <= 7, t <= 3 that the reference's defaults and t = 1 produce: (3,1), (4,1),
 * (5,1), (5,2), (6,1), (6,2), (7,1), (7,2), (7,3) -- FFGPU_ENOTSUP otherwise, and for unaligned rows (compose the
 * layer from ffgpu_gate_rng_batch / ffgpu_gf256_mask_open / ffgpu_gf256_bits_affine_fold then).  Randomness: as
 * ffgpu_gate_rng_batch (host key + nonce + rounds, or dev_state with `nonce` as offset and defer_advance; with
 * defer_advance = 0 the launch advances the device-resident nonce itself).  For t = 1 and more than three words per
 * thread of the (capped) grid, a thread's keystream continues from word to word: the coefficient a given position
 * receives then depends on n and on the number of compute units -- as with every device-CSPRNG entry point, the
 * randomness is not part of the parity contract (the opened values are).  Scalars: canonical 2-limb host scalars.  */
int ffgpu_gf256_sbox_layer(ffgpu_ctx* ctx, const uint64_t* host_matrix, const uint64_t* host_bias, const uint64_t* host_lambda,
                           const uint64_t* host_mu, int t, int m, const void* x, size_t x_stride, const void* rbits,
                           size_t rbits_stride, void* out, size_t out_stride, size_t n, const uint8_t* host_key32, uint64_t nonce,
                           int rounds, void* dev_state, int defer_advance, void* stream);

/* out[h] = A * bits(in[h]^254) + B packed back to a byte, with the 8x8 GF(2)
 * matrix given as 8 row bytes (bit c of host_rows8[r] = A[r][c]) and B as a byte.
 * replaces: demos/np_aes.py:37-43 sbox() evaluated on public values.           */
int ffgpu_gf256_sbox(ffgpu_ctx* ctx, const void* in, const uint8_t* host_rows8, uint8_t b,
                     void* out, size_t n, void* stream);

/* ---- timing helper ------------------------------------------------------ */
/* Runs `reps` back-to-back launches of ffgpu_mul on `stream` bracketed by HIP
 * events on that stream and returns the mean milliseconds per launch.
 * (bench-side convenience; equivalent entry points exist for split/recombine) */
int ffgpu_time_mul(ffgpu_ctx* ctx, const void* a, const void* b, void* out, size_t n,
                   int reps, void* stream, float* ms_per_launch);
int ffgpu_time_split(ffgpu_ctx* ctx, const void* secrets, const void* coeffs, size_t coeff_stride,
                     int t, int m, void* shares, size_t share_stride, size_t n,
                     int reps, void* stream, float* ms_per_launch);
int ffgpu_time_recombine(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda,
                         int k, int w, void* out, size_t out_stride, size_t n,
                         int reps, void* stream, float* ms_per_launch);
/* device-to-device copy of `bytes` (multiple of 16, 16-byte aligned) with the library's own
 * streaming kernel: the achievable-bandwidth yardstick reported next to the 8 TB/s nominal peak. */
int ffgpu_copy(ffgpu_ctx* ctx, const void* src, void* dst, size_t bytes, void* stream);
/* VALU issue-rate yardstick (the compute-side counterpart of ffgpu_time_copy): what the chip sustains for one instruction
 * kind -- op 0: v_bitop3_b32, 1: v_add_u32, 2: v_mad_u64_u32, 3: v_xor_b32, 4: v_perm_b32, 5: v_lshrrev_b32, 6: v_and_or_b32,
 * 7: v_add3_u32, 8: v_mul_lo_u32, 9: v_alignbit_b32 (rotate), 10: v_lshl_or_b32, 11: v_alignbyte_b32, 12: v_lshrrev_b64, 13: v_lshl_add_u64 -- with `waves_per_simd` waves on every SIMD and `iters` x 128
 * instructions in 8 independent dependent-chains per wave.  out3[0] = lane-operations per second (events around the launch),
 * out3[1] = shader clock in MHz under that load (s_memtime against the 100 MHz counter), out3[2] = shader cycles per wave
 * instruction and SIMD.  scratch32: 32 bytes of device memory.  bench.py prices its VALU-bound rows with it.
 * SYNCHRONISES `stream` (event wait + a blocking read-back of the cycle counts): not legal during stream capture, unlike
 * the computing entry points.
 * replaces: nothing in the reference (measurement aid, like the ffgpu_time_* entry points).                            */
int ffgpu_valu_probe(ffgpu_ctx* ctx, int op, int iters, int waves_per_simd, void* scratch32, double* out3, void* stream);
int ffgpu_time_copy(ffgpu_ctx* ctx, const void* src, void* dst, size_t bytes,
                    int reps, void* stream, float* ms_per_launch);

/* ---- device-side wire: share rows between CO-LOCATED party processes -------------------------------------
 * The reference marshals every share row with pickle.dumps and moves the bytes through its asyncio TCP mesh
 * (runtime.py:484-495, 655-661, 571-577; asyncoro.py:54-106): at n = 10^7 that is 80 MB per row and message, 0.5-0.7 s
 * per gate among three local parties against 0.4 ms of kernels.  When the parties are processes on one node (one per
 * GPU, or several on one GPU) the row need not leave the device: the exporting party sends a 64-byte interprocess
 * handle + offset instead of the limb bytes, the receiving party opens it and copies device-to-device (over xGMI
 * between GPUs).  The host side (mpyc_amd/ipcwire.py) keeps the exported buffer alive until every receiver has
 * acknowledged its copy.
 *   export: synchronises `stream` (the row is complete), returns the handle of the ALLOCATION that contains ptr and
 *           ptr's offset in it (hipMemGetAddressRange + hipIpcGetMemHandle);
 *   open:   maps the exporter's allocation into this process (hipIpcOpenMemHandle; not valid in the exporting
 *           process itself -- the host side short-circuits that case); close unmaps it;
 *   read:   copies `bytes` from base + offset into dst and synchronises `stream`.
 *   canary: export also returns the first and last 16 bytes of the row (canary32, may be NULL); read, given them
 *           (expect_canary32, may be NULL), compares them with what the mapping shows BEFORE copying and returns
 *           FFGPU_ESTALE on a mismatch -- the guard for mappings a receiver keeps cached across messages, should an
 *           exporter ever free an allocation and obtain the same handle bytes for a new one.
 * replaces: pickle.dumps(row) / pickle.loads(bytes) of the np path for co-located parties.                      */
#define FFGPU_IPC_HANDLE_BYTES 64
int ffgpu_ipc_export(ffgpu_ctx* ctx, const void* ptr, size_t bytes, unsigned char* handle, unsigned long long* offset,
                     unsigned char* canary32, void* stream);
int ffgpu_ipc_open(ffgpu_ctx* ctx, const unsigned char* handle, void** base);
int ffgpu_ipc_read(ffgpu_ctx* ctx, const void* base, unsigned long long offset, void* dst, size_t bytes,
                   const unsigned char* expect_canary32, void* stream);
/* read + ffgpu_reduce in ONE pass: n field elements are read through the mapping, reduced to canonical form (a peer's data
 * must be canonical before any kernel computes on it, as `field.array(unmarshal(r))` guarantees at runtime.py:508, 677)
 * and written to dst; synchronises `stream`. */
int ffgpu_ipc_read_reduced(ffgpu_ctx* ctx, const void* base, unsigned long long offset, void* dst, size_t n,
                           const unsigned char* expect_canary32, void* stream);
int ffgpu_ipc_close(ffgpu_ctx* ctx, void* base);

#ifdef __cplusplus
}
#endif
#endif /* FFGPU_H */
