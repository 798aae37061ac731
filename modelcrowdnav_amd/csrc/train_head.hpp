// train_head.hpp -- the head that the value networks' training kernels end in (sarl_train.hip: SARL's mlp3 on
// [self state | pooled feature]; value_train.hip: CADRL's value_network on a 13-wide row and LSTM-RL's mlp on
// [self state | h_N]): the MLP IN -> 150 -> 100 -> 100 -> 1 once per state, with the MSE loss.  Here are its place in the
// flat buffers, its LDS buffers and the one function that runs it forwards, forms the loss and runs it backwards.  The
// precision rules live here alone: a float64 forward pass whose float32 copies feed a float32 backward pass, and the loss,
// d loss / d v and the gradient of the last bias formed in float64 and rounded once.
//
// world_train.hip keeps its own mlp3 on purpose.  It runs once per pedestrian with mlp3.0 applied as two column blocks,
// has two outputs and a forward-only mode, and borrows the trunk's float64 buffers: head_step would need a switch for each
// of the four, which costs more than the copy.
#pragma once
#include "train_linear.hpp"    // NT, lin_fwd, lin_bwd_x, lin_bwd_w

namespace {

// ---- the MLP the value networks end in: IN -> 150 -> 100 -> 100 -> 1, ReLU between the layers
struct HeadOffsets {
    int w[4], b[4];             // float offsets of each layer's weight and bias in the flat buffers
};
HeadOffsets head_offsets(int at, int IN)
{
    const int in[4] = {IN, 150, 100, 100}, out[4] = {150, 100, 100, 1};
    HeadOffsets h;
    for (int l = 0; l < 4; ++l) {
        h.w[l] = at; at += in[l] * out[l];
        h.b[l] = at; at += out[l];
    }
    return h;
}
constexpr int head_floats(int IN) { return IN * 150 + 150 + 150 * 100 + 100 + 100 * 100 + 100 + 100 + 1; }

// LDS elements per state: the activations in float64 and their float32 copies, two backward buffers, target, d loss / d v
constexpr int HEAD_STATE_DOUBLES = 152 + 100 + 100 + 1;
constexpr int HEAD_STATE_FLOATS = 152 + 100 + 100 + 152 + 152 + 2;

struct Head {
    double *M1d, *M2d, *M3d, *Vd;
    float *M1, *M2, *M3, *U0, *U1, *Yt, *DV;
};
__device__ __forceinline__ Head carve_head(double *&d64, float *&f32, int G)
{
    auto taked = [&d64](int n) { double *q = d64; d64 += n; return q; };
    auto take = [&f32](int n) { float *q = f32; f32 += n; return q; };
    Head h;
    h.M1d = taked(G * 152), h.M2d = taked(G * 100), h.M3d = taked(G * 100), h.Vd = taked(G);
    h.M1 = take(G * 152), h.M2 = take(G * 100), h.M3 = take(G * 100), h.U0 = take(G * 152), h.U1 = take(G * 152);
    h.Yt = take(G), h.DV = take(G);
    return h;
}

// Forward pass of the MLP on the Gc inputs X[g][0 .. IN) (float32 or float64, row stride ldx), this group's sums of the
// squared errors and of d loss / d v = 2 (v - y) / B into ws_sums, then the backward pass: each layer's partial gradient
// into the workgroup's slice gP, from the float32 copy Xf of the input.  With WANT_DX it leaves d loss / d X in
// h.U1[g * 152 + i] and ends on a barrier.  The caller has synchronised after writing X, Xf and h.Yt.
template <typename TX, bool WANT_DX>
__device__ __forceinline__ void head_step(const float *__restrict__ P, float *__restrict__ gP, const HeadOffsets &of,
                                          const TX *X, int ldx, const float *Xf, int ldxf, int IN, const Head &h, int Gc,
                                          int B, double *__restrict__ ws_sums)
{
    lin_fwd<TX, false, true>(P + of.w[0], IN, P + of.b[0], X, ldx, 1, h.M1d, 152, h.M1, 152, Gc, IN, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[1], 150, P + of.b[1], h.M1d, 152, 1, h.M2d, 100, h.M2, 100, Gc, 150, 100);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[2], 100, P + of.b[2], h.M2d, 100, 1, h.M3d, 100, h.M3, 100, Gc, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[3], 100, P + of.b[3], h.M3d, 100, 1, h.Vd, 1, nullptr, 0, Gc, 100, 1);
    __syncthreads();

    if (threadIdx.x == 0) {                                 // the loss, float64
        double acc = 0.0, dsum = 0.0;
        for (int g = 0; g < Gc; ++g) {
            const double d = h.Vd[g] - (double)h.Yt[g];
            const double dv = 2.0 * d / (double)B;
            acc += d * d;
            dsum += dv;
            h.DV[g] = (float)dv;
        }
        ws_sums[2 * blockIdx.x] = acc;
        ws_sums[2 * blockIdx.x + 1] = dsum;                 // the gradient of the last bias, before any float32 rounding
    }
    __syncthreads();

    lin_bwd_w(h.DV, 1, h.M3, 100, 1, gP + of.w[3], 100, gP + of.b[3], Gc, 100, 1);
    lin_bwd_x<false>(P + of.w[3], 100, h.DV, 1, h.U0, 152, h.M3, 100, Gc, 100, 1);
    __syncthreads();
    lin_bwd_w(h.U0, 152, h.M2, 100, 1, gP + of.w[2], 100, gP + of.b[2], Gc, 100, 100);
    lin_bwd_x<false>(P + of.w[2], 100, h.U0, 152, h.U1, 152, h.M2, 100, Gc, 100, 100);
    __syncthreads();
    lin_bwd_w(h.U1, 152, h.M1, 152, 1, gP + of.w[1], 150, gP + of.b[1], Gc, 150, 100);
    lin_bwd_x<false>(P + of.w[1], 150, h.U1, 152, h.U0, 152, h.M1, 152, Gc, 150, 100);
    __syncthreads();
    lin_bwd_w(h.U0, 152, Xf, ldxf, 1, gP + of.w[0], IN, gP + of.b[0], Gc, IN, 150);
    if (WANT_DX) {
        lin_bwd_x<false>(P + of.w[0], IN, h.U0, 152, h.U1, 152, nullptr, 0, Gc, IN, 150);
        __syncthreads();
    }
}

}  // namespace
