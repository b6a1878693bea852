/*
 * ffgpu_math.h -- second header of libffgpu.so: the local steps under the secure logarithm and exponential of fixed-point
 * numbers (runtime.np_log, np_exp2 and their wrappers, runtime.py:4853-4945), under the probabilistic zero test over a
 * Blum prime (runtime._np_is_zero, runtime.py:3581-3620), under secure random bits (runtime.np_random_bits,
 * runtime.py:4187-4273), under the secure binary sign by Legendre symbols (demos/np_bnnmnist.py:44-156) and under secure unit
 * vectors and table lookup at secret indices (runtime.np_unit_vector, unit_vector, runtime.py:4979-5029) that no entry of
 * ffgpu.h serves, and the local correlation of a secure 2-D convolution layer (demos/np_cnnmnist.py:53-85).  Same library, same contexts (ffgpu_ctx of ffgpu.h), same
 * conventions:
 *   - every entry returns an int status of ffgpu.h (FFGPU_OK == 0); nothing throws across the boundary;
 *   - array arguments are DEVICE pointers unless the name says host; elements are canonical little-endian limbs in the
 *     layouts ffgpu.h lists, host scalars little-endian 64-bit limbs, ffgpu_ctx_scalar_limbs() of them;
 *   - `stream` is a hipStream_t passed as void*; calls are asynchronous on it, allocate nothing and never synchronise (they
 *     can be captured in a HIP graph); inputs are never written, outputs are canonical;
 *   - n == 0 returns FFGPU_OK whatever the pointers (the counts are still checked); in every refused case nothing is
 *     written and nothing is launched;
 *   - an output that overlaps an input is FFGPU_EINVAL (the exceptions are stated at ffgm_powers_prod and ffgm_rbits_finish);
 *   - prime fields only: FFGPU_ENOTSUP for a GF(2^n) context; every element size (4, 8, 12, 16, 24 bytes) -- but for the two
 *     Keccak entries at the end, which serve GF(2^n <= 8) only.
 * The entries carry the prefix ffgm_ .  protocols.py composes them, with the entries of ffgpu.h, into powers(), log(),
 * log2(), log10(), pow_public_base(), exp2() and exp(), into is_zero() and equal(), into random_bits(), into bsgn() and into
 * demux(), random_unit_vectors(), unit_vectors(), unit_vectors_from_bits() and lookup(), and into keccak_f1600(), sponge(),
 * sha3() and shake(), and into conv2d() and conv_layer().
 *
 * A block of powers is POWER-MAJOR: row j holds y^(j+1) for the n elements, rows `stride` >= n elements apart.
 *
 * ffgm_powers_prod: out[j*n + e] = P[(h-1)*stride + e] * P[j*stride + e] for j < w, 1 <= w <= h -- the top power of a block
 *   of h powers times its w lowest: the local (degree-2t) products of one doubling step of the power ladder, dense (w, n).
 *   A thread keeps the top power in registers across its w products: w + 1 loads per element.  `out` may lie in the same
 *   allocation as P from row h on (past the h rows read: at or after P + ((h-1)*stride + n) elements); any overlap with the
 *   h rows read, padding between them included, is FFGPU_EINVAL.
 *   replaces: runtime.py:4966-4967 (`b[:, -1:] * c`, the broadcast product before its re-sharing).
 * ffgm_poly_dot: out[e] = c0 + sum_{j<theta} tab[j] * P[j*stride + e], 1 <= theta <= 64.  tab: a device table of theta
 *   canonical elements (public coefficients), host_c0: one canonical host scalar.  One lazy accumulation and one reduction
 *   per element; (theta + 1) * n elements of traffic.
 *   replaces: runtime.py:4887 and :4934 (`ys @ coefficients` for public coefficients, runtime.py:2513-2531, and the constant).
 * ffgm_pow_base: out[e] = g^((x[e] >> shift) mod 2^ebits) with x[e] taken as its canonical integer; the caller guarantees
 *   x[e] >> shift < 2^ebits.  tab: the fixed-base window table of g, 15 * ceil(ebits/4) canonical elements,
 *   tab[15*i + d - 1] = g^(d * 16^i) for d = 1..15.  At most ceil(ebits/4) - 1 products per element and no squarings; the
 *   table is staged in LDS per workgroup.  1 <= ebits <= bit_length(p), 0 <= shift < 192.
 *   replaces: runtime.py:1408 and :1422 (gmpy2.powmod_exp_list with a public base) and the shift at :1421.
 * ffgm_bits_reverse: out[h*l + j] = bits[h*l + l-1-j] for the element-major (n, l) bits of ffgpu_bits_finish, 1 <= l <= 64.
 *   replaces: runtime.py:4876 (np_flip along the bit axis).
 *
 * The masked copies of the zero test are ROW-MAJOR (k, n): row i holds the i-th copy of the n elements, rows n elements
 * apart (the layout ffgpu_prod_rows consumes); count = k*n entries.  A code is one BYTE per entry.
 *
 * ffgm_iszero_mask: out[i*n + e] = a[e]*r[i*n + e] + (1 - 2*z[i*n + e])*u2[i*n + e] for i < k, k >= 1.  z holds SHARES of
 *   bits (arbitrary field elements): two full products per entry, accumulated lazily, one reduction.  A thread keeps its
 *   elements of `a` in registers across the k rows: (4k + 1)*n elements of traffic.
 *   replaces: runtime.py:3608 (`a * r + (1 - (z << 1)) * u2`, the broadcast of a over the k rows included).
 * ffgm_legendre_code: code[j] = 2 if c[j] == 0, else 1 if c[j]^((p-1)/2) == 1 (a quadratic residue), else 0.  The
 *   exponentiation is the one ffgpu_pow launches for this exponent; only the ends differ.  p odd: FFGPU_ENOTSUP for p == 2.
 *   replaces: finfields.py:1464-1470 (is_sqr: the Legendre symbols by gmpy2.legendre) and the test `c == 0` of runtime.py:3614.
 * ffgm_iszero_finish: out[j] = z[j] if code[j] == 0, 1 - z[j] if code[j] == 1, 1 if code[j] == 2 (0 counts as a square).
 *   replaces: runtime.py:3614-3615 (`np.where(c == 0, 0, z)`, `np.where(is_sqr, 1 - z, z)` and the 1 of a zero).
 *
 * The rows of the random-bit entries are SEPARATE arrays of n entries: host_r, host_z, host_b are host arrays of device
 * pointers, one per row; at most 64 rows (the limit of ffgpu_recombine), whole packs in ffgm_rbits_open for up to 9.
 *
 * ffgm_rbits_open: out[h] = sum_{i<k} lambda[i] * (r_i[h]^2 + z_i[h]); *zeros += #{h : out[h] == 0}.  host_lambda: k host
 *   scalars (the Lagrange vector of the k = 2t+1 senders).  The squares are reduced products, the sum is accumulated lazily
 *   with one reduction per entry: 2k rows read, one written.  zeros: a device int32 that is ADDED to (one atomic per wave
 *   that saw a zero), or NULL.
 *   replaces: runtime.py:4251-4254 (`_r.value**2 + z.value`, its opening at threshold 2t, and the count of `_r2 != 0`).
 * ffgm_rbits_finish: with s = c[h]^((3p-5)/4), the inverse square root of a square modulo p = 3 mod 4:
 *   b_i[h] = r_i[h] * s * 2^f (is_signed: +-1 scaled) or (r_i[h] * s + 1) * (p+1)/2 * 2^f (0 or 1 scaled) for i < m, and 0 in
 *   every row where c[h] == 0.  The exponentiation of the public c runs once for all m rows and is the one ffgpu_pow
 *   launches for this exponent.  b_i may BE r_i (the same pointer); any other overlap of a b_i with c, an r_j or a b_j is
 *   FFGPU_EINVAL.  c is never written.  0 <= f < 192.
 *   replaces: runtime.py:4265-4272 (`r * field.array._sqrt(r2, INV=True)`, finfields.py:1424-1437, the `+ 1`, the halving
 *   and the shift), once per party.
 *
 * The arrays of the binary sign are ROW-MAJOR (w, n), rows n elements apart, 1 <= w <= 8: row i belongs to the i-th symbol.
 *
 * ffgm_bsgn_mask: out[i*n + e] = z[i*n + e] * (alpha*a[e] + beta[i]) for i < w.  host_alpha: one host scalar, host_beta: w of
 *   them, canonical.  A thread forms alpha*a once and keeps it in registers across the w rows; per row one addition, one
 *   lazy product, one reduction: (2w + 1)*n elements of traffic.
 *   replaces: np_bnnmnist.py:72, :106-110 and :147-150 (`y * (2*a + 1)`, `y + [[-2], [0], [2]]` and its broadcast product).
 * ffgm_bsgn_finish: c: the public opened (w, n) values; host_s, host_out: host arrays of m <= 64 device pointers, party q's
 *   (w, n) shares of the signs and its output.  With h = (c[i*n + e] | p), which is 1, -1 or 0:
 *     sum == 0: out_q[i*n + e] = h * s_q[i*n + e] (s, p - s or 0), w*n entries;
 *     sum == 1: out_q[e] = sum_{i<w} h_i * s_q[i*n + e], n entries.
 *   The exponentiation by (p-1)/2 is the one ffgpu_pow launches for this exponent and runs once per opened value for all m
 *   parties; no codes are written.  p odd: FFGPU_ENOTSUP for p == 2.
 *   replaces: np_bnnmnist.py:74, :113-114 and :154 (`s * legendre_p(y)`, gmpy2.legendre per entry, and the sum over the rows).
 *
 * Unit vectors are POSITION-MAJOR (rows, n): row j holds position j for the n secret indices, rows n elements apart -- the
 * (outer = 1, k = rows, inner = n) layout ffgpu_tour_unit_expand and ffgpu_matmul take as it is.  K2 = 2^kbits.
 *
 * ffgm_unit_prod: out[j*n + e] = x[e*xstride] * U[j*n + e] for j < h, h >= 1 -- the broadcast product of a demultiplexer
 *   round, dense (h, n): bit x of every index times the h rows so far (degree 2t, before its re-sharing;
 *   ffgpu_tour_unit_expand interleaves (u - v, v) after it).  A thread keeps its x in registers across the h rows: h + 1 loads
 *   per element.  xstride = 1 for a row of random bits, xstride = l for one bit position of the element-major (n, l) bits of
 *   ffgpu_bits_finish (x then points at that position of element 0).
 *   replaces: random.py:141-151 (`x[i] * u` and its broadcast) and runtime.py:4993-4996 (scalar_mul(x[i], u)).
 * ffgm_unit_roll: out[j*n + e] = U[((j - c[e]) mod K2)*n + e] for j < K, 1 <= K <= K2, 0 <= kbits <= 30 -- the (K2, n) random
 *   unit vectors rotated down by the opened public offsets, the first K rows kept.  c: canonical elements; c[e] mod K2 is
 *   taken from the low kbits bits of the canonical integer.  A gather: U is read by element.
 *   replaces: runtime.py:5026-5028 (`c.value % n` and np.roll(u, c)), per index.
 * ffgm_unit_dot: out[e] = sum_{j<rows} tab[(j + c[e]) mod K2] * U[j*n + e] -- a table read through unit vectors that are never
 *   rotated.  tab: a device table of tlen canonical elements (public values or a party's shares: the arithmetic is the same),
 *   entries from tlen up count as 0.  With c: rows == K2 and 1 <= tlen <= K2.  c == NULL: no rotation, tab[j], any rows >= 1,
 *   tlen == rows, kbits is not looked at.  The table is staged in LDS, one word per entry: at most 64 KiB, so with c
 *   kbits <= 14, 13, 12, 12, 11 for elements of 4, 8, 12, 16, 24 bytes (without c: rows <= 2^that); beyond: FFGPU_ENOTSUP.
 *   One lazy accumulation per element, reduced every 192 terms (32 for the multi-limb 2^k - c primes); one store per element.
 *   replaces: runtime.py:5016 (`u @ np.arange(n)`, any public table in its place) and `T @ np_unit_vector(a, n)` of the callers.
 *
 * The tensors of a convolution layer are dense and ROW-MAJOR: x (k, r, m, n) -- k images of r input channels, m rows, n
 * columns --, W (v, r, s, s), b (v), out (k, v, m, n).  host_x, host_w, host_b, host_out are host arrays of nsend <= 64 device
 * pointers, sender q's tensors; host_b == NULL: no bias (else every entry is set).
 *
 * ffgm_conv2d: out_q[i, j, I, J] = b_q[j] + sum_{l<r} sum_{di<s} sum_{dj<s} x_q[i, l, I + di - (s-1)/2, J + dj - s/2] * W_q[j, l, di, dj]
 *   for q < nsend, terms whose x index falls outside [0, m) x [0, n) being 0; 1 <= s <= 16 and s <= n (m < s is fine).  The two
 *   offsets differ for even s: the row offset is the demo's s2, the column offset np.correlate(mode='same')'s.  One launch
 *   for all senders; a workgroup owns one image, one tile of output pixels and one block of output channels and keeps its
 *   sums in registers, reduced every 192 terms (32 for the multi-limb 2^k - c primes) after whole filter rows.  Traffic: x
 *   once per block of output channels, W once per tile, out once; no scratch: memory linear in the tensors.  Inputs may
 *   alias each other (the same public W for every sender); an output overlapping any input or another output is
 *   FFGPU_EINVAL.  k*v*m*n == 0 with valid counts: FFGPU_OK, nothing launched.
 *   replaces: np_cnnmnist.py:69-80 (the four nested loops around np.correlate on object arrays, and the bias).
 * ffgm_conv2d_plan: host-only, launches nothing: the shape ffgm_conv2d takes for these sizes on this context -- the tile,
 *   the output channels per workgroup, the input channels per staging step, the grid, the LDS bytes, the filter rows
 *   between two reductions, and whether it is the wide shape.  Refuses what ffgm_conv2d refuses for the same counts.
 *
 * FFGPU_OK: n == 0 / count == 0.  FFGPU_EINVAL: a null context or required pointer; h < 1, w < 1 or w > h; theta < 1 or
 * theta > 64; ebits < 1 or ebits > bit_length(p), shift < 0 or shift >= 192; l < 1 or l > 64; stride < n; k < 1; m < 1;
 * f < 0 or f >= 192; w < 1 or w > 8; sum not 0 or 1; xstride < 1; kbits < 0 or kbits > 30; K < 1 or K > K2; rows != K2 with c,
 * tlen != rows without, tlen < 1 or tlen > K2; nsend < 1, s < 1, s > 16 or s > n, r, m, n or v < 1 with a non-empty output;
 * a size overflowing (rows * n included); an output overlapping an input or another output.
 * FFGPU_ENOTSUP: a GF(2^n) context; ffgm_legendre_code and ffgm_bsgn_finish over p == 2; ffgm_rbits_finish unless
 * p = 3 mod 4; more than 64 rows or parties; a table of ffgm_unit_dot beyond 64 KiB of LDS; more than 64 senders or a grid beyond HIP's limit in ffgm_conv2d.        */
#ifndef FFGPU_MATH_H
#define FFGPU_MATH_H

#include "ffgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

int ffgm_powers_prod(ffgpu_ctx* ctx, const void* P, size_t stride, int h, int w, void* out, size_t n, void* stream);
int ffgm_poly_dot(ffgpu_ctx* ctx, const void* P, size_t stride, int theta, const void* tab, const uint64_t* host_c0, void* out, size_t n,
                  void* stream);
int ffgm_pow_base(ffgpu_ctx* ctx, const void* x, int shift, int ebits, const void* tab, void* out, size_t n, void* stream);
int ffgm_bits_reverse(ffgpu_ctx* ctx, const void* bits, int l, void* out, size_t n, void* stream);
int ffgm_iszero_mask(ffgpu_ctx* ctx, const void* a, const void* r, const void* z, const void* u2, int k, void* out, size_t n,
                     void* stream);
int ffgm_legendre_code(ffgpu_ctx* ctx, const void* c, uint8_t* code, size_t count, void* stream);
int ffgm_iszero_finish(ffgpu_ctx* ctx, const uint8_t* code, const void* z, void* out, size_t count, void* stream);
int ffgm_rbits_open(ffgpu_ctx* ctx, const void* const* host_r, const void* const* host_z, const uint64_t* host_lambda, int k, void* out,
                    int32_t* zeros, size_t n, void* stream);
int ffgm_rbits_finish(ffgpu_ctx* ctx, const void* c, const void* const* host_r, void* const* host_b, int m, int is_signed, int f, size_t n,
                      void* stream);
int ffgm_bsgn_mask(ffgpu_ctx* ctx, const void* a, const void* z, const uint64_t* host_alpha, const uint64_t* host_beta, int w, void* out,
                   size_t n, void* stream);
int ffgm_bsgn_finish(ffgpu_ctx* ctx, const void* c, const void* const* host_s, void* const* host_out, int m, int w, int sum, size_t n,
                     void* stream);
int ffgm_unit_prod(ffgpu_ctx* ctx, const void* x, size_t xstride, const void* U, size_t h, void* out, size_t n, void* stream);
int ffgm_unit_roll(ffgpu_ctx* ctx, const void* U, const void* c, int kbits, size_t K, void* out, size_t n, void* stream);
int ffgm_unit_dot(ffgpu_ctx* ctx, const void* U, size_t rows, const void* c, int kbits, const void* tab, size_t tlen, void* out, size_t n,
                  void* stream);

typedef struct ffgm_conv2d_plan_t {
    int tile_rows, tile_cols;   /* output pixels of a workgroup's tile */
    int out_channels;           /* output channels of a workgroup */
    int in_channels_step;       /* input channels staged in LDS per step */
    int flush_rows;             /* filter rows between two reductions of an accumulator */
    int wide;                   /* 1: the wide shape, 0: the narrow one */
    size_t grid_x, grid_y;      /* workgroups: k * tiles * channel blocks, senders (0, 0 for an empty output) */
    size_t lds_bytes;           /* dynamic LDS of a workgroup */
} ffgm_conv2d_plan_t;
int ffgm_conv2d(ffgpu_ctx* ctx, const void* const* host_x, const void* const* host_w, const void* const* host_b, void* const* host_out,
                int nsend, size_t k, size_t r, size_t m, size_t n, size_t v, int s, void* stream);
int ffgm_conv2d_plan(ffgpu_ctx* ctx, size_t k, size_t r, size_t m, size_t n, size_t v, int s, int nsend, ffgm_conv2d_plan_t* host_plan);

/* ---- threshold SHA-3: secure rounds of Keccak-f[1600] (demos/sha3.py:72-106) over GF(2^n), 1 <= n <= 8 ------------------
 * The ONE exception to "prime fields only": these two entries serve GF(2^n <= 8) contexts and no other.
 * Every bit of a 1600-bit Keccak state is shared as one element (one byte) of the context's field.  A party's share of a
 * batch of `nstates` states is nstates x 1600 bytes, state-major: position i = 64 (5 y + x) + z of state b (S[i] of
 * sha3.py:43, A[x, y, z]) is byte 1600 b + i.  One round for one sender's share a:
 *   1. a = sum_{s<k} lambda_s rows[s] (k = 1, lambda = 1: a plain share); iota_round >= 0: the field's 1 is added at
 *      z = 2^j - 1 of plane (0, 0) for the set bits j < 7 of that round's constant (sha3.py:31-33, 102-103);
 *   2. theta, rho, pi (sha3.py:85-95);   3. chi's local product out = b + (b[x+1] + 1) b[x+2] (sha3.py:98): degree 2t.
 * ffgm_gf2_keccak_local writes `out` of that map (apply_round = 1) or the state after step 1 only (apply_round = 0: the
 *   tail after round 23, a plain recombination) for `nbatch` senders in one launch: sender y reads every row
 *   batch_stride_in bytes x y further on and writes at out + y * batch_stride_out.  Deterministic.
 * ffgm_gf2_keccak_round is the same map for the senders 1..2t+1 followed by the share generation of `_reshare`
 *   (runtime.py:603-689, thresha.py:47-64) for each of the 1600 elements, coefficients from the device CSPRNG: the
 *   share of party j+1 from sender y goes to shares + j * share_stride + y * batch_stride_out -- the [recipient][sender]
 *   block of ffgpu_gate_rng_batch.  Randomness as ffgpu_gate_rng_batch (host key + nonce < 2^40 + rounds, or dev_state with
 *   `nonce` as offset and defer_advance); the keystream a position receives depends on (key, nonce, sender, state index,
 *   position) only, never on nstates.  (m, t) = (1, 0) writes the round's output as the one party's share.
 * All strides in bytes.  FFGPU_ENOTSUP with nothing written: a context that is not GF(2^n <= 8), k > 7, (m, t) other than
 * (1, 0) and the nine pairs of ffgpu_gf256_sbox_layer, 2^n <= m, row pointers or strides that are not multiples of 4,
 * iota_round outside -1..23.  Scalars: canonical 2-limb host scalars.                                                   */
int ffgm_gf2_keccak_local(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, size_t batch_stride_in,
                           int nbatch, int iota_round, int apply_round, void* out, size_t batch_stride_out, size_t nstates,
                           void* stream);
int ffgm_gf2_keccak_round(ffgpu_ctx* ctx, const void* const* host_rows, const uint64_t* host_lambda, int k, size_t batch_stride_in,
                           int iota_round, const uint8_t* host_key32, uint64_t nonce, int rounds, void* dev_state,
                           int defer_advance, int t, int m, void* shares, size_t share_stride, size_t batch_stride_out,
                           size_t nstates, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* FFGPU_MATH_H */
