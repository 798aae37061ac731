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
//   train_grad_reduce_kernel      (train_reduce.hpp) sums the slices in workgroup order into the flat gradient and
//                                 writes the loss (the only writer of `loss`; without a gradient it writes nothing else).
//   adam_kernel                   torch.optim.Adam (no weight decay, no amsgrad) over the flat buffers.
//
// The layout, the precision rules and the autograd semantics are those of sarl_train.hip, whose trunk
// (train_attention.hpp) and layer helpers (train_linear.hpp) this file shares: flat float32 buffers in state_dict order,
// a float64 forward pass whose float32 copies feed a float32 backward pass, float64 sums over the batch rounded once, the
// un-stabilised masked softmax with NaN where torch has NaN, and attention.4.bias with a gradient of exactly 0 (or NaN).
//
// Where the activations live.  Up to ROWS_IN_LDS = 16 rows per workgroup everything is in LDS (145 668 B at 16 rows).
// From 17 pedestrians on -- one scene per workgroup, up to MCN_MAX_HUMANS = 32 rows -- the float64 row buffers and
// mlp3's float32 activations (which are per pedestrian here, not per state) are the workgroup's own piece of the
// workspace instead, and LDS holds the rest (139 652 B at 32 rows).
#include "train_attention.hpp"  // the layer table and the trunk; NT, lin_fwd, lin_bwd_*
#include "train_reduce.hpp"     // the grouping and the reduce kernel

namespace {

constexpr int D = 4;        // a pedestrian's input: px, py, vx, vy
constexpr int DOUT = 2;     // and output: the next vx, vy

TrainOffsets world_offsets() { return train_offsets(D, D + 50, DOUT); }     // mlp3 on [own state | pooled feature] -> vx, vy

// elements per row and per scene: the trunk's and, carved by the kernel around them, this head's (the gathered input,
// the targets and the outputs' gradient; the pooled feature and its gradient)
constexpr int ROW_FLOATS = D + 2 * DOUT + TRUNK_ROW_FLOATS;   // always in LDS
constexpr int ROW_FLOATS_M3 = 152 + 100 + 100;                // mlp3's activations: LDS, or the workspace
constexpr int ROW_DOUBLES = TRUNK_ROW_DOUBLES;                // float64 forward buffers: LDS, or the workspace
constexpr int STATE_FLOATS = TRUNK_STATE_FLOATS + 52 + 52;
constexpr int STATE_DOUBLES = TRUNK_STATE_DOUBLES + 52;
constexpr int ROWS_IN_LDS = 16;
constexpr int LDS_DOUBLES = 18210;                            // 145 680 B: 16 rows of one scene with everything in LDS, 12 B to spare

bool rows_in_lds(int N) { return group_states(N) * N <= ROWS_IN_LDS; }
bool group_fits(int G, int N)
{
    const long rows = (long)G * N;
    const long d = (long)G * STATE_DOUBLES + (rows_in_lds(N) ? rows * ROW_DOUBLES : 0);
    const long f = rows * ROW_FLOATS + (long)G * STATE_FLOATS + (rows_in_lds(N) ? rows * ROW_FLOATS_M3 : 0);
    return 8 * d + 4 * f <= 8L * LDS_DOUBLES && rows <= 32;
}

__global__ __launch_bounds__(NT) void attn_world_loss_grad_kernel(const float *__restrict__ P, TrainOffsets of,
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
    double *st64 = lds;
    double *row64 = ws_rows64 ? ws_rows64 + (size_t)blockIdx.x * Rcap * ROW_DOUBLES : lds + (size_t)G * STATE_DOUBLES;
    float *at = reinterpret_cast<float *>(lds + (size_t)G * STATE_DOUBLES + (ws_rows64 ? 0 : (size_t)Rcap * ROW_DOUBLES));
    auto take = [&at](int n) { float *q = at; at += n; return q; };
    float *X = take(Rcap * D), *Yt = take(Rcap * DOUT), *DO = take(Rcap * DOUT);
    const Trunk t = carve_trunk(st64, row64, at, G, Rcap);
    double *PLd = st64;                     // [G][52], after the trunk's
    float *PL = take(G * 52), *DP = take(G * 52);
    if (ws_rows32) at = ws_rows32 + (size_t)blockIdx.x * Rcap * ROW_FLOATS_M3;
    float *M1 = take(Rcap * 152), *M2 = take(Rcap * 100), *M3 = take(Rcap * 100);
    // the head's float64 layer buffers are the trunk's, free once it has run; the outputs take the feature's place once
    // it is pooled.  Its backward layer buffers are the trunk's too.
    double *const Td = t.Td, *const Ud = t.Ud, *const Hd = t.Hd, *const OUTd = t.FEATd;
    float *const T0 = t.T0, *const T1 = t.T1;

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
    trunk_forward(P, of, X, D, D, t, Gc, N, R);
    for (int it = tid; it < Gc * 50; it += NT) {                        // pooled feature of the scene
        const int g = it / 50, j = it - g * 50;
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc = fma(t.WTd[g * N + n], t.FEATd[(g * N + n) * 52 + j], acc);
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

    for (int it = tid; it < Gc * 50; it += NT) {                        // the expansion backwards: summed over the scene
        const int g = it / 50, j = it - g * 50;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += T1[(g * N + n) * 152 + j];
        DP[g * 52 + j] = acc;
    }
    __syncthreads();

    // ---- the trunk: pooling, softmax, attention, the mean, mlp2, mlp1
    trunk_backward(P, gP, of, X, D, D, DP, 52, t, Gc, N, R);
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

// one slice of every parameter's partial gradient per workgroup, four float64 per workgroup for its sums, and above
// ROWS_IN_LDS rows per workgroup its float64 row buffers and mlp3 activations
long attn_world_train_workspace_floats(int B, int N)
{
    const long groups = train_groups(B, N);
    const long rows = (long)group_states(N) * N;
    return slice_floats(groups, world_offsets().total) + 8 * groups +
           (rows_in_lds(N) ? 0 : groups * rows * (2 * ROW_DOUBLES + ROW_FLOATS_M3));
}

int launch_attn_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int B,
                                int N, void *workspace, float *grad, float *loss, hipStream_t stream)
{
    const TrainOffsets of = world_offsets();
    const int G = group_states(N);
    const long groups = train_groups(B, N);
    if (!group_fits(G, N) || groups > 0x7fffffffL / (of.total + 1)) return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + slice_floats(groups, of.total));
    double *ws_rows64 = rows_in_lds(N) ? nullptr : ws_sums + 4 * groups;
    float *ws_rows32 = rows_in_lds(N) ? nullptr : reinterpret_cast<float *>(ws_rows64 + groups * G * N * ROW_DOUBLES);
    hipLaunchKernelGGL(attn_world_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, cur, nxt, rows,
                       B, N, G, grad ? 1 : 0, ws, ws_sums, ws_rows64, ws_rows32);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    return launch_train_grad_reduce(ws, ws_sums, groups, of.total, 4, of.b[L3D], DOUT, (double)B * (double)(N * DOUT), grad,
                                    loss, stream);
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
