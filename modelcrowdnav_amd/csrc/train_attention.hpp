// train_attention.hpp -- what the training kernels of the two attention networks (sarl_train.hip: the SARL value network,
// world_train.hip: the AttentionWorld world model) have in common.  Both networks are the same trunk -- mlp1, the mean
// over the crowd (global state), mlp2, attention, the un-stabilised masked softmax -- under a different head: mlp3 once per
// state on [self state | pooled feature] with one output, or once per pedestrian on [own state | pooled feature] with two.
// Here are the layer table of the flat buffers and the trunk's buffers with its forward and backward pass; the grouping of
// a batch into workgroups and the kernel that sums their slices are in train_reduce.hpp.  Each .hip keeps its gather, its
// LDS budget and its optimizer; SARL's head and loss are train_head.hpp's (shared with value_train.hip), the world model's
// per-pedestrian head and loss are its own.
#pragma once
#include "launch.hpp"
#include "train_linear.hpp"    // NT, CH, lin_fwd, lin_bwd_x, lin_bwd_w

namespace {

// ---- the flat parameter / gradient buffers: state_dict order, each weight row-major [out][in] as torch holds it
constexpr int NLAYER = 11;
enum { L1A, L1B, L2A, L2B, LTA, LTB, LTC, L3A, L3B, L3C, L3D };

struct TrainOffsets {
    int w[NLAYER], b[NLAYER];   // float offsets of each layer's weight and bias in the flat buffers
    int total;
};

// D: a row's input width; J: the width of mlp3.0's input; OUT: the width of the network's output
TrainOffsets train_offsets(int D, int J, int OUT)
{
    const int in[NLAYER] = {D, 150, 100, 100, 200, 100, 100, J, 150, 100, 100};
    const int out[NLAYER] = {150, 100, 100, 50, 100, 100, 1, 150, 100, 100, OUT};
    TrainOffsets t;
    int at = 0;
    for (int l = 0; l < NLAYER; ++l) {
        t.w[l] = at; at += in[l] * out[l];
        t.b[l] = at; at += out[l];
    }
    t.total = at;
    return t;
}

// ---- the trunk's buffers.  Float64: what the forward pass hands from layer to layer; float32: the copies the backward
// pass reads, and its temporaries.  Elements per row (one human of one state) and per state, as carve_trunk takes them;
// a kernel adds its head's own to these and budgets its LDS by the sums.
constexpr int TRUNK_ROW_DOUBLES = 100 + 52 + 152 + 100 + 3;
constexpr int TRUNK_STATE_DOUBLES = 100;
constexpr int TRUNK_ROW_FLOATS = 152 + 100 + 100 + 52 + 100 + 100 + 52 + 152 + 152 + 100 + 4;
constexpr int TRUNK_STATE_FLOATS = 100 + 100 + 1;

struct Trunk {
    double *GMd;                                        // per state: the global state
    double *Hd, *FEATd, *Td, *Ud, *Sd, *Ed, *WTd;       // per row: mlp1's output, feature, two layer buffers, score, e, weight
    float *H1, *H, *F1, *FEAT, *A1, *A2;                // per row: the activations mlp1.0, mlp1.2, mlp2.0, mlp2.2, attention.0, .2
    float *DF, *T0, *T1, *DH;                           // per row, backward: d feature, two layer buffers, d (mlp1's output)
    float *S, *WT, *DWT, *DS;                           // per row: score, weight and their gradients
    float *GM, *DG, *ZS;                                // per state: global state, its gradient, the share of attention.4.bias
};
// Once the trunk's forward pass is done a head may use Td, Ud, Hd and FEATd (after pooling) as its own float64 layer
// buffers, and before the trunk's backward pass T0 and T1: the backward pass reads none of them.

// Takes the trunk's buffers for G states of Rcap = G N rows from three cursors and moves them on: the float64 buffers of
// the states, those of the rows (the caller points this one at LDS or at the workgroup's piece of the workspace), and
// the float32 buffers.
__device__ __forceinline__ Trunk carve_trunk(double *&state64, double *&row64, float *&f32, int G, int Rcap)
{
    auto taked = [](double *&at, int n) { double *q = at; at += n; return q; };
    auto take = [&f32](int n) { float *q = f32; f32 += n; return q; };
    Trunk t;
    t.GMd = taked(state64, G * 100);
    t.Hd = taked(row64, Rcap * 100), t.FEATd = taked(row64, Rcap * 52), t.Td = taked(row64, Rcap * 152);
    t.Ud = taked(row64, Rcap * 100), t.Sd = taked(row64, Rcap), t.Ed = taked(row64, Rcap), t.WTd = taked(row64, Rcap);
    t.H1 = take(Rcap * 152), t.H = take(Rcap * 100), t.F1 = take(Rcap * 100), t.FEAT = take(Rcap * 52);
    t.A1 = take(Rcap * 100), t.A2 = take(Rcap * 100), t.DF = take(Rcap * 52), t.T0 = take(Rcap * 152);
    t.T1 = take(Rcap * 152), t.DH = take(Rcap * 100);
    t.S = take(Rcap), t.WT = take(Rcap), t.DWT = take(Rcap), t.DS = take(Rcap);
    t.GM = take(G * 100), t.DG = take(G * 100), t.ZS = take(G);
    return t;
}

// Forward pass of the trunk on the R = Gc N gathered rows X[r][0 .. D) (row stride ldx), float64 from layer to layer.
// Leaves Hd, FEATd, WTd (per row) and GMd (per state) with their float32 copies, and the other float32 activations the
// backward pass reads.  The caller has synchronised after writing X; the trunk ends on a barrier.
__device__ __forceinline__ void trunk_forward(const float *__restrict__ P, const TrainOffsets &of, const float *X, int ldx,
                                              int D, const Trunk &t, int Gc, int N, int R)
{
    const int tid = threadIdx.x;
    lin_fwd<float, false, true>(P + of.w[L1A], D, P + of.b[L1A], X, ldx, 1, t.Td, 152, t.H1, 152, R, D, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L1B], 150, P + of.b[L1B], t.Td, 152, 1, t.Hd, 100, t.H, 100, R, 150, 100);
    __syncthreads();
    for (int it = tid; it < Gc * 100; it += NT) {                       // global state: mean over the humans
        const int g = it / 100, j = it - g * 100;
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc += t.Hd[(g * N + n) * 100 + j];
        t.GMd[it] = acc / (double)N;
        t.GM[it] = (float)t.GMd[it];
    }
    lin_fwd<double, false, true>(P + of.w[L2A], 100, P + of.b[L2A], t.Hd, 100, 1, t.Td, 152, t.F1, 100, R, 100, 100);
    lin_fwd<double, false, false>(P + of.w[LTA], 200, P + of.b[LTA], t.Hd, 100, 1, t.Ud, 100, nullptr, 0, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[L2B], 100, P + of.b[L2B], t.Td, 152, 1, t.FEATd, 52, t.FEAT, 52, R, 100, 50);
    lin_fwd<double, true, true>(P + of.w[LTA] + 100, 200, nullptr, t.GMd, 100, N, t.Ud, 100, t.A1, 100, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[LTB], 100, P + of.b[LTB], t.Ud, 100, 1, t.Td, 152, t.A2, 100, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[LTC], 100, P + of.b[LTC], t.Td, 152, 1, t.Sd, 1, t.S, 1, R, 100, 1);
    __syncthreads();
    if (tid < Gc) {                                                     // masked softmax, literally
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            const int r = tid * N + n;
            const double sc = t.Sd[r];
            t.Ed[r] = exp(sc) * (sc != 0.0 ? 1.0 : 0.0);
            sum += t.Ed[r];
        }
        for (int n = 0; n < N; ++n) {
            t.WTd[tid * N + n] = t.Ed[tid * N + n] / sum;
            t.WT[tid * N + n] = (float)t.WTd[tid * N + n];
        }
    }
    __syncthreads();
}

// Backward pass of the trunk, plain float32: from DP[g * ldp + j], j < 50, the gradient with respect to state g's pooled
// feature sum_n weight_n feature_n, through the pooling, the masked softmax, attention, the mean, mlp2 and mlp1, each
// layer's partial gradient into the workgroup's slice gP.  The caller has synchronised after writing DP.
__device__ __forceinline__ void trunk_backward(const float *__restrict__ P, float *__restrict__ gP, const TrainOffsets &of,
                                               const float *X, int ldx, int D, const float *DP, int ldp, const Trunk &t,
                                               int Gc, int N, int R)
{
    const int tid = threadIdx.x;
    // ---- pooling and softmax
    for (int it = tid; it < R * 50; it += NT) {                         // d feature = weight * d pooled
        const int r = it / 50, j = it - r * 50;
        t.DF[r * 52 + j] = t.WT[r] * DP[(r / N) * ldp + j];
    }
    for (int r = tid; r < R; r += NT) {                                 // d weight = <d pooled, feature>
        float acc = 0.f;
        for (int j = 0; j < 50; ++j) acc = fmaf(DP[(r / N) * ldp + j], t.FEAT[r * 52 + j], acc);
        t.DWT[r] = acc;
    }
    __syncthreads();
    if (tid < Gc) {
        // w = e / sum, e = exp(s) mask.  Autograd's chain d e_n = d w_n / sum - sum_k d w_k e_k / sum^2,
        // d s_n = d e_n mask_n exp(s_n) is, with the factors collected, d s_n = w_n (d w_n - sum_k d w_k w_k): the same
        // numbers without the cancellation between two quotients, exactly 0 for a single human (w = 1) and for a masked
        // one (w = 0), and NaN for a state whose sum is 0 (w = NaN), as autograd's.
        float dot = 0.f;
        for (int n = 0; n < N; ++n) dot = fmaf(t.DWT[tid * N + n], t.WT[tid * N + n], dot);
        int m = -1;                                     // the participant (w != 0, or NaN) with the largest |d s|
        for (int n = 0; n < N; ++n) {
            const int r = tid * N + n;
            t.DS[r] = t.WT[r] * (t.DWT[r] - dot);
            if (!(t.WT[r] == 0.f) && (m < 0 || fabsf(t.DS[r]) > fabsf(t.DS[tid * N + m]))) m = n;
        }
        // The weights of a state sum to 1, so its d s sum to 0: a common shift of the scores (attention.4.bias) has no
        // gradient.  Rounding leaves 1e-10 of it.  The constraint is kept instead: the others are summed (float64, rounded
        // once) and the largest d s is set to minus that sum, which moves it by the rounding residue of the formula above;
        // the state's share of attention.4.bias is that sum plus that d s: 0 exactly, or NaN.
        float zs = 0.f;
        if (m >= 0) {
            double others = 0.0;
            for (int n = 0; n < N; ++n)
                if (n != m) others += (double)t.DS[tid * N + n];
            const float of32 = (float)others;
            t.DS[tid * N + m] = -of32;
            zs = of32 + t.DS[tid * N + m];
        }
        t.ZS[tid] = zs;
    }
    __syncthreads();
    if (tid == 0) {
        float acc = 0.f;
        for (int g = 0; g < Gc; ++g) acc += t.ZS[g];
        gP[of.b[LTC]] = acc;
    }

    // ---- attention
    lin_bwd_w(t.DS, 1, t.A2, 100, 1, gP + of.w[LTC], 100, nullptr, R, 100, 1);
    lin_bwd_x<false>(P + of.w[LTC], 100, t.DS, 1, t.T0, 152, t.A2, 100, R, 100, 1);
    __syncthreads();
    lin_bwd_w(t.T0, 152, t.A1, 100, 1, gP + of.w[LTB], 100, gP + of.b[LTB], R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTB], 100, t.T0, 152, t.T1, 152, t.A1, 100, R, 100, 100);
    __syncthreads();
    lin_bwd_w(t.T1, 152, t.H, 100, 1, gP + of.w[LTA], 200, gP + of.b[LTA], R, 100, 100);
    lin_bwd_w(t.T1, 152, t.GM, 100, N, gP + of.w[LTA] + 100, 200, nullptr, R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTA], 200, t.T1, 152, t.DH, 100, nullptr, 0, R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTA] + 100, 200, t.T1, 152, t.T0, 152, nullptr, 0, R, 100, 100);   // d (expanded global state)
    __syncthreads();
    for (int it = tid; it < Gc * 100; it += NT) {                       // expand and mean, backwards
        const int g = it / 100, j = it - g * 100;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += t.T0[(g * N + n) * 152 + j];
        t.DG[it] = acc / (float)N;
    }
    __syncthreads();
    for (int it = tid; it < R * 100; it += NT) {
        const int r = it / 100, j = it - r * 100;
        t.DH[it] += t.DG[(r / N) * 100 + j];
    }
    __syncthreads();

    // ---- mlp2
    lin_bwd_w(t.DF, 52, t.F1, 100, 1, gP + of.w[L2B], 100, gP + of.b[L2B], R, 100, 50);
    lin_bwd_x<false>(P + of.w[L2B], 100, t.DF, 52, t.T0, 152, t.F1, 100, R, 100, 50);
    __syncthreads();
    lin_bwd_w(t.T0, 152, t.H, 100, 1, gP + of.w[L2A], 100, gP + of.b[L2A], R, 100, 100);
    lin_bwd_x<true>(P + of.w[L2A], 100, t.T0, 152, t.DH, 100, t.H, 100, R, 100, 100);           // + ReLU of mlp1.2
    __syncthreads();

    // ---- mlp1
    lin_bwd_w(t.DH, 100, t.H1, 152, 1, gP + of.w[L1B], 150, gP + of.b[L1B], R, 150, 100);
    lin_bwd_x<false>(P + of.w[L1B], 150, t.DH, 100, t.T1, 152, t.H1, 152, R, 150, 100);
    __syncthreads();
    lin_bwd_w(t.T1, 152, X, ldx, 1, gP + of.w[L1A], D, gP + of.b[L1A], R, D, 150);
}

}  // namespace
