// conv2d.hpp -- the 2-D correlation of a batch of images with a bank of filters over a prime field, all senders of a secure
// convolution layer in one kernel (the loops of the demo's convolvetensor, np_cnnmnist.py:69-80).  Included by kernels.hpp
// after unitvec.hpp.
#pragma once
#include "conv2d_geom.hpp"

namespace ffgpu {

// the tensors of the senders of one launch: sender q (blockIdx.y) reads x[q], w[q], b[q] (null: no bias), writes out[q]
template <class F>
struct Conv2dArgs {
    const typename F::elem* x[CONV2D_MAX_SENDERS];
    const typename F::elem* w[CONV2D_MAX_SENDERS];
    const typename F::elem* b[CONV2D_MAX_SENDERS];
    typename F::elem* out[CONV2D_MAX_SENDERS];
};

// bytes of one staged operand: the word, or its 28-bit digits for the policies with a digit accumulator
template <class F>
constexpr size_t conv2d_slot_bytes() {
    return DotAcc<F>::lazy ? (size_t)DotAcc<F>::NL * sizeof(uint32_t) : sizeof(typename F::word);
}

// Y[i, j, I, J] = b[j] + sum_{l, di, dj} x[i, l, I + di - (s-1)/2, J + dj - s/2] W[j, l, di, dj].  Geometry, index
// arithmetic and the flush schedule: conv2d_geom.hpp.  Direct and output-stationary, the inner operation k_convolve's: the
// policy's lazily reduced multiply-accumulate (DotSum: acc_mac, or 28-bit digit columns for the multi-limb 2^k - c primes,
// whose operands are staged in LDS as digits, the window digit-major), reduced after every conv2d_flush_rows() filter
// rows.  The taps are the constant operand: f.prep.  The lanes of a wave read ONE tap per step (same address: LDS
// broadcast) and consecutive window elements of a tile row; a lane keeps VR outputs in registers, so a window element is
// read once for VR products.  Memory: a tile reads its window of x once per block of VB output channels and W once per
// tile (both from cache after the first), writes its outputs once with the default cache policy; no scratch, no partial
// sums outside the thread.  LDS: g.CH channels of window and taps, dynamic (conv2d_lds_bytes).
template <class F, class S>
__global__ __launch_bounds__(BLOCK) void k_conv2d(F f, Conv2dArgs<F> a, Conv2dGeom g) {
    typedef typename F::word W;
    typedef typename F::elem E;
    static_assert((int)S::THREADS == (int)BLOCK, "Conv2dShape is laid out for the library's workgroup");
    constexpr bool LZ = DotAcc<F>::lazy;
    constexpr int NL = DotAcc<F>::NL;
    constexpr int VR = S::VR;
    extern __shared__ __attribute__((aligned(16))) unsigned char conv2d_smem[];
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.y;
    const E* __restrict__ x = a.x[q];
    const E* __restrict__ w = a.w[q];
    const E* __restrict__ bias = a.b[q];
    E* __restrict__ out = a.out[q];
    const Conv2dBlock bl = conv2d_block(g, blockIdx.x);
    const Conv2dLane ln = conv2d_lane(g, tid);
    const int s = g.s, ss = s * s;
    const int win_one = g.WH * g.WW, tap_one = S::VB * ss;
    const int win_all = g.CH * win_one, tap_all = g.CH * tap_one;        // the slots of a full step: the LDS layout
    W* Ws = reinterpret_cast<W*>(conv2d_smem);                           // words: window, then taps
    W* Ts = Ws + win_all;
    uint32_t* Wd = reinterpret_cast<uint32_t*>(conv2d_smem);             // digits: window digit-major, then taps digit-minor
    uint32_t* Td = Wd + (size_t)NL * win_all;
    const int period = conv2d_flush_rows(s, DotAcc<F>::FLUSH);
    DotSum<F> acc[VR];
#pragma unroll
    for (int u = 0; u < VR; ++u) acc[u].zero(f);
    bool have = false;
    int rows_since = 0;
    for (size_t l0 = 0; l0 < g.r; l0 += (size_t)g.CH) {
        const int nch = g.r - l0 < (size_t)g.CH ? (int)(g.r - l0) : g.CH;
        for (int i = tid; i < nch * win_one; i += BLOCK) {
            int cl, wy, wx;
            conv2d_win_of(g, i, cl, wy, wx);
            const int64_t row = conv2d_win_row(bl.I0, wy, s), col = conv2d_win_col(bl.J0, wx, s);
            const bool ok = conv2d_in_image(row, col, g.m, g.n);        // outside: read the image's first element, then zero it
            const W val = ff_keep_if<W>(ld_elem<F>(x, conv2d_x_index(g, bl.img, l0 + (size_t)cl, ok ? (size_t)row : 0, ok ? (size_t)col : 0)), ok);
            if constexpr (LZ) {
                uint32_t d[NL];
                f.lacc_digits(val, d);
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) Wd[t_ * win_all + i] = d[t_];
            } else {
                Ws[i] = val;
            }
        }
        for (int i = tid; i < nch * tap_one; i += BLOCK) {
            int cl, c, tap;
            conv2d_tap_of(g, i, cl, c, tap);
            const size_t j = bl.j0 + (size_t)c;
            const bool ok = j < g.v;                                    // channels past v: read W's first element, then zero it
            const W val = ff_keep_if<W>(f.prep(ld_elem<F>(w, ok ? conv2d_w_index(g, j, l0 + (size_t)cl, tap) : 0)), ok);
            if constexpr (LZ) {
                uint32_t d[NL];
                f.lacc_digits(val, d);
#pragma unroll
                for (int t_ = 0; t_ < NL; ++t_) Td[i * NL + t_] = d[t_];
            } else {
                Ts[i] = val;
            }
        }
        __syncthreads();
        for (int cl = 0; cl < nch; ++cl) {
            for (int di = 0; di < s; ++di) {
                const int wrow = conv2d_win_slot(g, cl, ln.py + di, ln.px);
                const int trow = conv2d_tap_slot(g, cl, ln.c0, di, 0);
                for (int dj = 0; dj < s; ++dj) {
                    if constexpr (LZ) {
                        uint32_t xd[NL];
#pragma unroll
                        for (int t_ = 0; t_ < NL; ++t_) xd[t_] = Wd[t_ * win_all + wrow + dj];
#pragma unroll
                        for (int u = 0; u < VR; ++u) {
                            uint32_t td[NL];
#pragma unroll
                            for (int t_ = 0; t_ < NL; ++t_) td[t_] = Td[(trow + u * ss + dj) * NL + t_];
                            acc[u].mac_digits(f, td, xd);
                        }
                    } else {
                        const W xv = Ws[wrow + dj];
#pragma unroll
                        for (int u = 0; u < VR; ++u) acc[u].mac(f, Ts[trow + u * ss + dj], xv);
                    }
                }
                if (++rows_since == period) {               // keep the unreduced accumulators inside their headroom
#pragma unroll
                    for (int u = 0; u < VR; ++u) acc[u].flush(f, have);
                    have = true;
                    rows_since = 0;
                }
            }
        }
        __syncthreads();
    }
    const size_t I = bl.I0 + (size_t)ln.py, J = bl.J0 + (size_t)ln.px;
#pragma unroll
    for (int u = 0; u < VR; ++u) {
        const size_t j = bl.j0 + (size_t)(ln.c0 + u);
        if (I < g.m && J < g.n && j < g.v) {
            W y = acc[u].result(f, have);
            if (bias) y = f.add(y, ld_elem<F>(bias, j));
            st_elem<F>(out, conv2d_y_index(g, bl.img, j, I, J), y);
        }
    }
}

}  // namespace ffgpu
