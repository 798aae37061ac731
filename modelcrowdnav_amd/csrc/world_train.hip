// world_train.hip -- one training step of the AttentionWorld world model (policy/world_model.py, the default shape:
// input_dim 4, global state on) without autograd: MSE loss and its gradient for a mini-batch, and the Adam update.
//
//   attn_world_loss_grad_kernel   one workgroup per G scenes (at most 8 rows, or one scene; a row is one pedestrian of one
//                                 scene).  It gathers its rows of the pair memory, runs the forward pass with the
//                                 activations kept for the backward pass, forms its share of the loss and, unless only
//                                 the loss is asked for, back-propagates through mlp3 (per pedestrian), the pooling, the
//                                 masked softmax, attention, the mean (global state), mlp2 and mlp1.  Its gradient of
//                                 EVERY parameter goes into its own slice of the workspace: no atomics, no workgroup
//                                 looks at another one's data.
//   attn_world_grad_reduce_kernel sums the slices in workgroup order into the flat gradient and writes the loss (the only
//                                 writer of `loss`; without a gradient it writes nothing else).
//   adam_kernel                   torch.optim.Adam (no weight decay, no amsgrad) over the flat buffers.
//
// The layout, the precision rules and the autograd semantics are those of sarl_train.hip, whose layer helpers
// (train_linear.hpp) this file shares: flat float32 buffers in state_dict order, a float64 forward pass whose float32
// copies feed a float32 backward pass, float64 sums over the batch rounded once, the un-stabilised masked softmax with
// NaN where torch has NaN, and attention.4.bias with a gradient of exactly 0 (or NaN).
//
// Where the activations live.  Up to ROWS_IN_LDS = 16 rows per workgroup everything is in LDS (145 680 B at 16 rows).
// From 17 pedestrians on -- one scene per workgroup, up to MCN_MAX_HUMANS = 32 rows -- the float64 row buffers and
// mlp3's float32 activations (which are per pedestrian here, not per state) are the workgroup's own piece of the
// workspace instead, and LDS holds the rest (139 664 B at 32 rows).
#include <cstdio>
#include <cstdlib>
#include "launch.hpp"
#include "train_linear.hpp"    // NT, CH, lin_fwd, lin_bwd_x, lin_bwd_w

namespace {

constexpr int NLAYER = 11;
enum { L1A, L1B, L2A, L2B, LTA, LTB, LTC, L3A, L3B, L3C, L3D };
constexpr int D = 4;        // a pedestrian's input: px, py, vx, vy
constexpr int DOUT = 2;     // and output: the next vx, vy

struct WorldOffsets {
    int w[NLAYER], b[NLAYER];   // float offsets of each layer's weight and bias in the flat buffers
    int total;
};

WorldOffsets world_offsets()
{
    const int in[NLAYER] = {D, 150, 100, 100, 200, 100, 100, 50 + D, 150, 100, 100};
    const int out[NLAYER] = {150, 100, 100, 50, 100, 100, 1, 150, 100, 100, DOUT};
    WorldOffsets t;
    int at = 0;
    for (int l = 0; l < NLAYER; ++l) {
        t.w[l] = at; at += in[l] * out[l];
        t.b[l] = at; at += out[l];
    }
    t.total = at;
    return t;
}

// per row and per scene; the kernel carves its buffers by the same numbers
constexpr int ROW_FLOATS = D + 2 * DOUT + 152 + 100 + 100 + 52 + 100 + 100 + 52 + 152 + 152 + 100 + 4;   // always in LDS
constexpr int ROW_FLOATS_M3 = 152 + 100 + 100;                // mlp3's activations: LDS, or the workspace
constexpr int ROW_DOUBLES = 100 + 52 + 152 + 100 + 3;         // float64 forward buffers: LDS, or the workspace
constexpr int STATE_FLOATS = 100 + 52 + 100 + 52 + 4;
constexpr int STATE_DOUBLES = 100 + 52;
constexpr int ROWS_IN_LDS = 16;
constexpr int LDS_DOUBLES = 18210;                            // 145 680 B: 16 rows of one scene with everything in LDS

// scenes per workgroup: up to 8 rows for small crowds, one scene from 5 pedestrians on (N <= 32 rows)
int group_states(int N) { return N > 4 ? 1 : 8 / N; }
bool rows_in_lds(int N) { return group_states(N) * N <= ROWS_IN_LDS; }
bool group_fits(int G, int N)
{
    const long rows = (long)G * N;
    const long d = (long)G * STATE_DOUBLES + (rows_in_lds(N) ? rows * ROW_DOUBLES : 0);
    const long f = rows * ROW_FLOATS + (long)G * STATE_FLOATS + (rows_in_lds(N) ? rows * ROW_FLOATS_M3 : 0);
    return 8 * d + 4 * f <= 8L * LDS_DOUBLES && rows <= 32;
}

__global__ __launch_bounds__(NT) void attn_world_loss_grad_kernel(const float *__restrict__ P, WorldOffsets of,
                                                                  const float *__restrict__ cur,
                                                                  const float *__restrict__ nxt,
                                                                  const int64_t *__restrict__ rows, int B, int N, int G,
                                                                  int want_grad, float *__restrict__ ws,
                                                                  double *__restrict__ ws_sums, double *ws_rows64,
                                                                  float *ws_rows32)
{
    __shared__ double lds[LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    const int Gc = min(G, B - b0);          // scenes of this group (the last group may be short)
    const int R = Gc * N;                   // its rows
    float *const gP = ws + (size_t)blockIdx.x * of.total;

    const int Rcap = G * N;
    // float64 first (8-byte aligned), then the float32 buffers; with ws_rows64 / ws_rows32 the rows' float64 buffers and
    // mlp3's activations are this workgroup's own piece of the workspace instead
    double *atd = lds;
    auto taked = [&atd](int n) { double *q = atd; atd += n; return q; };
    double *GMd = taked(G * 100), *PLd = taked(G * 52);
    if (ws_rows64) atd = ws_rows64 + (size_t)blockIdx.x * Rcap * ROW_DOUBLES;
    double *Hd = taked(Rcap * 100), *FEATd = taked(Rcap * 52), *Td = taked(Rcap * 152), *Ud = taked(Rcap * 100);
    double *Sd = taked(Rcap), *Ed = taked(Rcap), *WTd = taked(Rcap);
    double *OUTd = FEATd;                   // the outputs take the feature's place once it is pooled
    float *at = reinterpret_cast<float *>(lds + (size_t)G * STATE_DOUBLES + (ws_rows64 ? 0 : (size_t)Rcap * ROW_DOUBLES));
    auto take = [&at](int n) { float *q = at; at += n; return q; };
    float *X = take(Rcap * D), *Yt = take(Rcap * DOUT), *DO = take(Rcap * DOUT), *H1 = take(Rcap * 152);
    float *H = take(Rcap * 100), *F1 = take(Rcap * 100), *FEAT = take(Rcap * 52), *A1 = take(Rcap * 100);
    float *A2 = take(Rcap * 100), *DF = take(Rcap * 52), *T0 = take(Rcap * 152), *T1 = take(Rcap * 152);
    float *DH = take(Rcap * 100), *S = take(Rcap), *WT = take(Rcap), *DWT = take(Rcap), *DS = take(Rcap);
    float *GM = take(G * 100), *PL = take(G * 52), *DG = take(G * 100), *DP = take(G * 52), *ZS = take(4 * G);
    if (ws_rows32) at = ws_rows32 + (size_t)blockIdx.x * Rcap * ROW_FLOATS_M3;
    float *M1 = take(Rcap * 152), *M2 = take(Rcap * 100), *M3 = take(Rcap * 100);

    // ---- gather: rows[b] (or b) picks the scene and its next velocities out of the pair memory
    for (int it = tid; it < R * D; it += NT) {
        const int g = it / (N * D), k = it - g * (N * D);
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[it] = cur[row * (N * D) + k];
    }
    for (int it = tid; it < R * DOUT; it += NT) {
        const int g = it / (N * DOUT), k = it - g * (N * DOUT);
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        Yt[it] = nxt[row * (N * DOUT) + k];
    }
    __syncthreads();

    // ---- forward (float64 from layer to layer; the float32 copies are what the backward pass reads)
    lin_fwd<float, false, true>(P + of.w[L1A], D, P + of.b[L1A], X, D, 1, Td, 152, H1, 152, R, D, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L1B], 150, P + of.b[L1B], Td, 152, 1, Hd, 100, H, 100, R, 150, 100);
    __syncthreads();
    for (int it = tid; it < Gc * 100; it += NT) {                       // global state: mean over the pedestrians
        const int g = it / 100, j = it - g * 100;
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc += Hd[(g * N + n) * 100 + j];
        GMd[it] = acc / (double)N;
        GM[it] = (float)GMd[it];
    }
    lin_fwd<double, false, true>(P + of.w[L2A], 100, P + of.b[L2A], Hd, 100, 1, Td, 152, F1, 100, R, 100, 100);
    lin_fwd<double, false, false>(P + of.w[LTA], 200, P + of.b[LTA], Hd, 100, 1, Ud, 100, nullptr, 0, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[L2B], 100, P + of.b[L2B], Td, 152, 1, FEATd, 52, FEAT, 52, R, 100, 50);
    lin_fwd<double, true, true>(P + of.w[LTA] + 100, 200, nullptr, GMd, 100, N, Ud, 100, A1, 100, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[LTB], 100, P + of.b[LTB], Ud, 100, 1, Td, 152, A2, 100, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[LTC], 100, P + of.b[LTC], Td, 152, 1, Sd, 1, S, 1, R, 100, 1);
    __syncthreads();
    if (tid < Gc) {                                                     // masked softmax, literally
        double sum = 0.0;
        for (int n = 0; n < N; ++n) {
            const int r = tid * N + n;
            const double sc = Sd[r];
            Ed[r] = exp(sc) * (sc != 0.0 ? 1.0 : 0.0);
            sum += Ed[r];
        }
        for (int n = 0; n < N; ++n) {
            WTd[tid * N + n] = Ed[tid * N + n] / sum;
            WT[tid * N + n] = (float)WTd[tid * N + n];
        }
    }
    __syncthreads();
    for (int it = tid; it < Gc * 50; it += NT) {                        // pooled feature of the scene
        const int g = it / 50, j = it - g * 50;
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc = fma(WTd[g * N + n], FEATd[(g * N + n) * 52 + j], acc);
        PLd[g * 52 + j] = acc;
        PL[g * 52 + j] = (float)acc;
    }
    // mlp3 on [own state | pooled feature], per pedestrian: the two column blocks of mlp3.0 one after the other
    lin_fwd<float, false, false>(P + of.w[L3A], 54, P + of.b[L3A], X, D, 1, Td, 152, nullptr, 0, R, D, 150);
    __syncthreads();
    lin_fwd<double, true, true>(P + of.w[L3A] + D, 54, nullptr, PLd, 52, N, Td, 152, M1, 152, R, 50, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L3B], 150, P + of.b[L3B], Td, 152, 1, Ud, 100, M2, 100, R, 150, 100);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L3C], 100, P + of.b[L3C], Ud, 100, 1, Hd, 100, M3, 100, R, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[L3D], 100, P + of.b[L3D], Hd, 100, 1, OUTd, DOUT, nullptr, 0, R, 100, DOUT);
    __syncthreads();

    // ---- loss: this group's sum of squared errors and of d loss / d out = 2 (out - y) / (B 2N), all float64
    if (tid == 0) {
        const double count = (double)B * (double)(N * DOUT);
        double acc = 0.0, dsum[DOUT] = {};
        for (int r = 0; r < R; ++r)
            for (int k = 0; k < DOUT; ++k) {
                const double d = OUTd[r * DOUT + k] - (double)Yt[r * DOUT + k];
                const double dv = 2.0 * d / count;
                acc += d * d;
                dsum[k] += dv;
                DO[r * DOUT + k] = (float)dv;
            }
        ws_sums[4 * blockIdx.x] = acc;
        for (int k = 0; k < DOUT; ++k) ws_sums[4 * blockIdx.x + 1 + k] = dsum[k];   // mlp3.6.bias, before any float32 rounding
    }
    if (!want_grad) return;                                             // forward only: the loss is all that is asked for
    __syncthreads();

    // ---- backward: mlp3 (mlp3.6.bias comes from the float64 sums above)
    lin_bwd_w(DO, DOUT, M3, 100, 1, gP + of.w[L3D], 100, nullptr, R, 100, DOUT);
    lin_bwd_x<false>(P + of.w[L3D], 100, DO, DOUT, T0, 152, M3, 100, R, 100, DOUT);
    __syncthreads();
    lin_bwd_w(T0, 152, M2, 100, 1, gP + of.w[L3C], 100, gP + of.b[L3C], R, 100, 100);
    lin_bwd_x<false>(P + of.w[L3C], 100, T0, 152, T1, 152, M2, 100, R, 100, 100);
    __syncthreads();
    lin_bwd_w(T1, 152, M1, 152, 1, gP + of.w[L3B], 150, gP + of.b[L3B], R, 150, 100);
    lin_bwd_x<false>(P + of.w[L3B], 150, T1, 152, T0, 152, M1, 152, R, 150, 100);
    __syncthreads();
    lin_bwd_w(T0, 152, X, D, 1, gP + of.w[L3A], 54, gP + of.b[L3A], R, D, 150);
    lin_bwd_w(T0, 152, PL, 52, N, gP + of.w[L3A] + D, 54, nullptr, R, 50, 150);
    lin_bwd_x<false>(P + of.w[L3A] + D, 54, T0, 152, T1, 152, nullptr, 0, R, 50, 150);   // d (expanded pooled feature)
    __syncthreads();

    // ---- pooling and softmax
    for (int it = tid; it < Gc * 50; it += NT) {                        // the expansion backwards: summed over the scene
        const int g = it / 50, j = it - g * 50;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += T1[(g * N + n) * 152 + j];
        DP[g * 52 + j] = acc;
    }
    __syncthreads();
    for (int it = tid; it < R * 50; it += NT) {                         // d feature = weight * d pooled
        const int r = it / 50, j = it - r * 50;
        DF[r * 52 + j] = WT[r] * DP[(r / N) * 52 + j];
    }
    for (int r = tid; r < R; r += NT) {                                 // d weight = <d pooled, feature>
        float acc = 0.f;
        for (int j = 0; j < 50; ++j) acc = fmaf(DP[(r / N) * 52 + j], FEAT[r * 52 + j], acc);
        DWT[r] = acc;
    }
    __syncthreads();
    if (tid < Gc) {
        // d s_n = w_n (d w_n - sum_k d w_k w_k), and the constraint sum_n d s_n = 0 kept exactly: sarl_train.hip has the
        // derivation.  The scene's share of attention.4.bias is 0 exactly, or NaN.
        float dot = 0.f;
        for (int n = 0; n < N; ++n) dot = fmaf(DWT[tid * N + n], WT[tid * N + n], dot);
        int m = -1;                                     // the participant (w != 0, or NaN) with the largest |d s|
        for (int n = 0; n < N; ++n) {
            const int r = tid * N + n;
            DS[r] = WT[r] * (DWT[r] - dot);
            if (!(WT[r] == 0.f) && (m < 0 || fabsf(DS[r]) > fabsf(DS[tid * N + m]))) m = n;
        }
        float zs = 0.f;
        if (m >= 0) {
            double others = 0.0;
            for (int n = 0; n < N; ++n)
                if (n != m) others += (double)DS[tid * N + n];
            const float of32 = (float)others;
            DS[tid * N + m] = -of32;
            zs = of32 + DS[tid * N + m];
        }
        ZS[tid] = zs;
    }
    __syncthreads();
    if (tid == 0) {
        float acc = 0.f;
        for (int g = 0; g < Gc; ++g) acc += ZS[g];
        gP[of.b[LTC]] = acc;
    }

    // ---- attention
    lin_bwd_w(DS, 1, A2, 100, 1, gP + of.w[LTC], 100, nullptr, R, 100, 1);
    lin_bwd_x<false>(P + of.w[LTC], 100, DS, 1, T0, 152, A2, 100, R, 100, 1);
    __syncthreads();
    lin_bwd_w(T0, 152, A1, 100, 1, gP + of.w[LTB], 100, gP + of.b[LTB], R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTB], 100, T0, 152, T1, 152, A1, 100, R, 100, 100);
    __syncthreads();
    lin_bwd_w(T1, 152, H, 100, 1, gP + of.w[LTA], 200, gP + of.b[LTA], R, 100, 100);
    lin_bwd_w(T1, 152, GM, 100, N, gP + of.w[LTA] + 100, 200, nullptr, R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTA], 200, T1, 152, DH, 100, nullptr, 0, R, 100, 100);
    lin_bwd_x<false>(P + of.w[LTA] + 100, 200, T1, 152, T0, 152, nullptr, 0, R, 100, 100);   // d (expanded global state)
    __syncthreads();
    for (int it = tid; it < Gc * 100; it += NT) {                       // expand and mean, backwards
        const int g = it / 100, j = it - g * 100;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += T0[(g * N + n) * 152 + j];
        DG[it] = acc / (float)N;
    }
    __syncthreads();
    for (int it = tid; it < R * 100; it += NT) {
        const int r = it / 100, j = it - r * 100;
        DH[it] += DG[(r / N) * 100 + j];
    }
    __syncthreads();

    // ---- mlp2
    lin_bwd_w(DF, 52, F1, 100, 1, gP + of.w[L2B], 100, gP + of.b[L2B], R, 100, 50);
    lin_bwd_x<false>(P + of.w[L2B], 100, DF, 52, T0, 152, F1, 100, R, 100, 50);
    __syncthreads();
    lin_bwd_w(T0, 152, H, 100, 1, gP + of.w[L2A], 100, gP + of.b[L2A], R, 100, 100);
    lin_bwd_x<true>(P + of.w[L2A], 100, T0, 152, DH, 100, H, 100, R, 100, 100);             // + ReLU of mlp1.2
    __syncthreads();

    // ---- mlp1
    lin_bwd_w(DH, 100, H1, 152, 1, gP + of.w[L1B], 150, gP + of.b[L1B], R, 150, 100);
    lin_bwd_x<false>(P + of.w[L1B], 150, DH, 100, T1, 152, H1, 152, R, 150, 100);
    __syncthreads();
    lin_bwd_w(T1, 152, X, D, 1, gP + of.w[L1A], D, gP + of.b[L1A], R, D, 150);
}

// loss = (sum of the workgroups' squared errors) / (B 2N), and with a gradient asked for grad[p] = sum over the
// workgroups' slices in index order.  The sums over the workgroups run in float64 and are rounded once; the order stays
// fixed.  mlp3.6.bias (the DOUT indices from bias_out) is summed from the workgroups' float64 sums of d loss / d out.
__global__ __launch_bounds__(256) void attn_world_grad_reduce_kernel(const float *__restrict__ ws,
                                                                     const double *__restrict__ ws_sums, int groups,
                                                                     int total, int bias_out, double count,
                                                                     float *__restrict__ grad, float *__restrict__ loss)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool from_sums = p >= bias_out && p < bias_out + DOUT;
    if (p == 0) {                                       // (thread 0 has a parameter of its own to sum as well)
        double acc = ws_sums[0];
        for (int g = 1; g < groups; ++g) acc += ws_sums[4 * g];
        *loss = (float)(acc / count);
    }
    if (!grad || p >= total) return;
    if (from_sums) {
        const int k = 1 + p - bias_out;
        double acc = ws_sums[k];
        for (int g = 1; g < groups; ++g) acc += ws_sums[4 * g + k];
        grad[p] = (float)acc;
    } else {
        double acc = ws[p];
        for (int g = 1; g < groups; ++g) acc += (double)ws[(size_t)g * total + p];
        grad[p] = (float)acc;
    }
}

// torch.optim.Adam (no weight decay, no amsgrad): m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g,
// p = p - step_size m / (sqrt(v) / bc2_sqrt + eps) with step_size = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t).
// Each element is worked out in float64 from the float32 state and rounded once per stored value.  g = 0 with zero
// moments gives m = v = 0 and p - 0 / eps: the parameter's own bits.
__global__ __launch_bounds__(256) void adam_kernel(float *__restrict__ p, float *__restrict__ m, float *__restrict__ v,
                                                   const float *__restrict__ grad, int64_t count, double beta1,
                                                   double beta2, double eps, double step_size, double bc2_sqrt)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        const double g = grad[i];
        const double mi = beta1 * (double)m[i] + (1.0 - beta1) * g;
        const double vi = beta2 * (double)v[i] + (1.0 - beta2) * g * g;
        m[i] = (float)mi;
        v[i] = (float)vi;
        p[i] = (float)((double)p[i] - step_size * mi / (sqrt(vi) / bc2_sqrt + eps));
    }
}

}  // namespace

namespace mcn {

long attn_world_train_param_count() { return world_offsets().total; }

// workgroups of the loss/gradient kernel for a batch of B scenes of N pedestrians
static long world_groups(int B, int N)
{
    const int G = group_states(N);
    return ((long)B + G - 1) / G;
}

// one slice of every parameter's partial gradient per workgroup (padded to whole float64s), four float64 per workgroup
// for its sums, and above ROWS_IN_LDS rows per workgroup its float64 row buffers and mlp3 activations
static long world_slice_floats(long groups, int total) { return (groups * total + 1) / 2 * 2; }
long attn_world_train_workspace_floats(int B, int N)
{
    const long groups = world_groups(B, N);
    const long rows = (long)group_states(N) * N;
    return world_slice_floats(groups, world_offsets().total) + 8 * groups +
           (rows_in_lds(N) ? 0 : groups * rows * (2 * ROW_DOUBLES + ROW_FLOATS_M3));
}

int launch_attn_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int B,
                                int N, void *workspace, float *grad, float *loss, hipStream_t stream)
{
    const WorldOffsets of = world_offsets();
    const int G = group_states(N);
    const long groups = world_groups(B, N);
    if (!group_fits(G, N) || groups > 0x7fffffffL / (of.total + 1)) return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + world_slice_floats(groups, of.total));
    double *ws_rows64 = rows_in_lds(N) ? nullptr : ws_sums + 4 * groups;
    float *ws_rows32 = rows_in_lds(N) ? nullptr : reinterpret_cast<float *>(ws_rows64 + groups * G * N * ROW_DOUBLES);
    hipLaunchKernelGGL(attn_world_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, cur, nxt, rows,
                       B, N, G, grad ? 1 : 0, ws, ws_sums, ws_rows64, ws_rows32);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    const unsigned blocks = grad ? (unsigned)((of.total + 255) / 256) : 1u;
    hipLaunchKernelGGL(attn_world_grad_reduce_kernel, dim3(blocks), dim3(256), 0, stream, ws, ws_sums, (int)groups, of.total,
                       of.b[L3D], (double)B * (double)(N * DOUT), grad, loss);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

// torch applies the hyper-parameters as the Python floats (float64) the user wrote -- 1e-3, 0.9, 0.999, 1e-8 -- and the C
// ABI carries them as float32, 5e-8 away.  That is enough to show: lr 0.001f in place of 0.001 moves every step by 5e-8 of
// itself, and on the recorded reference run (tests/golden/g20_trainer_sim.npz) that flipped one ReLU of one row at the
// sixth step, after which single weights were 2.6e-5 from the float64 replay instead of 8e-8.  So the float64 is
// recovered: the shortest decimal that rounds to the given float32, which is what was written for anything of up to 7
// digits.
static double written_as(float x)
{
    char buf[40];
    for (int digits = 1; digits <= 8; ++digits) {
        snprintf(buf, sizeof buf, "%.*e", digits - 1, (double)x);
        if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
    }
    return (double)x;
}

int launch_adam(float *params, float *exp_avg, float *exp_avg_sq, const float *grad, int64_t count, float lr, float beta1,
                float beta2, float eps, int step, hipStream_t stream)
{
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffLL) return MCN_EINVAL;
    const double b1 = written_as(beta1), b2 = written_as(beta2);
    const double step_size = written_as(lr) / (1.0 - pow(b1, (double)step));
    const double bc2_sqrt = sqrt(1.0 - pow(b2, (double)step));
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, params, exp_avg, exp_avg_sq, grad, count,
                       b1, b2, written_as(eps), step_size, bc2_sqrt);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace mcn
