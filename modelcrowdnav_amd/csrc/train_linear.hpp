// train_linear.hpp -- the linear-layer building blocks of the training kernels (sarl_train.hip, world_train.hip, world_mlp_train.hip, value_train.hip): the
// forward pass of one layer in float64 with float32 copies for the backward pass, and the two halves of its backward pass
// in float32.  A workgroup of NT threads works on R rows kept in LDS (or in its own piece of the workspace); the weights
// come from the flat parameter buffer, row-major [out][in] as torch holds them.
#pragma once
#include <hip/hip_runtime.h>

namespace {

constexpr int NT = 512;     // threads of a loss/gradient workgroup
constexpr int CH = 4;       // rows that one thread carries through a layer

// Y[r][o] = act(init + sum_i W[o][i] X[r / xdiv][i]) for r < R, o < OUT in float64; init = bias[o], or Y itself with ACCUM.
// Y goes out as float64 (Yd, the next layer's input) and, where Yf is given, as its float32 rounding for the backward pass.
// One thread carries CH rows of one output: W from global memory once per CH rows, X broadcast.
template <typename TX, bool ACCUM, bool RELU>
__device__ __noinline__ void lin_fwd(const float *__restrict__ W, int ldw, const float *__restrict__ bias, const TX *X,
                                     int ldx, int xdiv, double *Yd, int ldyd, float *Yf, int ldyf, int R, int IN, int OUT)
{
    const int nch = (R + CH - 1) / CH;
    for (int it = threadIdx.x; it < nch * OUT; it += NT) {
        const int c = it / OUT, o = it - c * OUT, r0 = c * CH;
        const float *w = W + o * ldw;
        const TX *xr[CH];
        double acc[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int r = min(r0 + k, R - 1);              // rows past the end repeat the last one and are not stored
            xr[k] = X + (r / xdiv) * ldx;
            acc[k] = ACCUM ? Yd[r * ldyd + o] : (double)bias[o];
        }
        double a1[CH] = {};                                // two interleaved chains per dot product
        int i = 0;
        for (; i + 2 <= IN; i += 2) {
            const double w0 = w[i], w1 = w[i + 1];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                acc[k] = fma(w0, (double)xr[k][i], acc[k]);
                a1[k] = fma(w1, (double)xr[k][i + 1], a1[k]);
            }
        }
        for (; i < IN; ++i) {
            const double wv = w[i];
#pragma unroll
            for (int k = 0; k < CH; ++k) acc[k] = fma(wv, (double)xr[k][i], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            double v = acc[k] + a1[k];
            if (RELU) v = v <= 0.0 ? 0.0 : v;              // NaN stays NaN, as torch's relu
            if (r0 + k < R) {
                Yd[(r0 + k) * ldyd + o] = v;
                if (Yf) Yf[(r0 + k) * ldyf + o] = (float)v;
            }
        }
    }
}

// dX[r][i] = (dX[r][i] with ACCUM) + sum_o dY[r][o] W[o][i], then zeroed where mask[r][i] <= 0 (the ReLU that made X).
// Lanes run along i: W is read coalesced.
template <bool ACCUM>
__device__ __noinline__ void lin_bwd_x(const float *__restrict__ W, int ldw, const float *dY, int ldy, float *dX,
                                       int ldx, const float *mask, int ldm, int R, int IN, int OUT)
{
    const int nch = (R + CH - 1) / CH;
    for (int it = threadIdx.x; it < nch * IN; it += NT) {
        const int c = it / IN, i = it - c * IN, r0 = c * CH;
        const float *dy[CH];
        float acc[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int r = min(r0 + k, R - 1);
            dy[k] = dY + r * ldy;
            acc[k] = ACCUM ? dX[r * ldx + i] : 0.f;
        }
        float a1[CH] = {}, a2[CH] = {}, a3[CH] = {};                 // four partial sums, as in lin_fwd
        int o = 0;
        for (; o + 4 <= OUT; o += 4) {
            const float w0 = W[o * ldw + i], w1 = W[(o + 1) * ldw + i], w2 = W[(o + 2) * ldw + i], w3 = W[(o + 3) * ldw + i];
#pragma unroll
            for (int k = 0; k < CH; ++k) {
                acc[k] = fmaf(dy[k][o], w0, acc[k]);
                a1[k] = fmaf(dy[k][o + 1], w1, a1[k]);
                a2[k] = fmaf(dy[k][o + 2], w2, a2[k]);
                a3[k] = fmaf(dy[k][o + 3], w3, a3[k]);
            }
        }
        for (; o < OUT; ++o) {
            const float wv = W[o * ldw + i];
#pragma unroll
            for (int k = 0; k < CH; ++k) acc[k] = fmaf(dy[k][o], wv, acc[k]);
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int r = r0 + k;
            const float v = (acc[k] + a1[k]) + (a2[k] + a3[k]);
            if (r < R) dX[r * ldx + i] = (mask && mask[r * ldm + i] <= 0.f) ? 0.f : v;
        }
    }
}

// gW[o][i] = sum_r dY[r][o] X[r / xdiv][i], gb[o] = sum_r dY[r][o] (gb may be NULL): this workgroup's partial gradient
// of one layer, rows in ascending order, written to its workspace slice.  (The three helpers are calls, not inlined:
// inlined into their thirty-odd call sites they cost the kernel its registers -- 1.6 KB of scratch per lane.)
__device__ __noinline__ void lin_bwd_w(const float *dY, int ldy, const float *X, int ldx, int xdiv,
                                       float *__restrict__ gW, int ldw, float *__restrict__ gb, int R, int IN, int OUT)
{
    for (int it = threadIdx.x; it < OUT * IN; it += NT) {
        const int o = it / IN, i = it - o * IN;
        float acc = 0.f;
        for (int r = 0; r < R; ++r) acc = fmaf(dY[r * ldy + o], X[(r / xdiv) * ldx + i], acc);
        gW[o * ldw + i] = acc;
    }
    if (gb)
        for (int o = threadIdx.x; o < OUT; o += NT) {
            float acc = 0.f;
            for (int r = 0; r < R; ++r) acc += dY[r * ldy + o];
            gb[o] = acc;
        }
}

}  // namespace
