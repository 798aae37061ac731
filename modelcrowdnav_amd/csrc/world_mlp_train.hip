// world_mlp_train.hip -- one training step of the MlpWorld world model (policy/world_model.py: 4N -> 128 -> 64 -> 12 ->
// 2N, ReLU after the first three layers, dropout after the first two, tanh on the output) without autograd: MSE loss and
// its gradient for a mini-batch.  The sum over the workgroups (train_reduce.hpp) and the Adam update (world_train.hip) are
// those of the AttentionWorld step, and so are the layout and the precision rules: flat float32 buffers in state_dict
// order, a float64 forward pass whose float32 copies feed a float32 backward pass, float64 sums over the batch rounded
// once, no atomics.
//
//   mlp_world_loss_grad_kernel   one workgroup per G = 8 scenes; a row is one scene, every activation is in LDS.  It
//                                gathers its rows of the pair memory, runs the forward pass (in train mode with the
//                                dropout masks of dropout_hash.hpp), forms its share of the loss and, unless only the loss
//                                is asked for, back-propagates into its own slice of the workspace.
//
// Dropout is multiplication by 0 or 1 / (1 - p), in both passes, after the ReLU's own select: a NaN or an infinity in a
// dropped unit comes out as NaN, as from nn.Dropout.  The backward pass keeps, per dropout layer, the ReLU's output (its
// select), the multiplier and the product (the next layer's input).
//
// Why G = 8.  One thread of lin_fwd / lin_bwd_x carries CH = 4 rows through a layer, and the time of a layer is the
// length of its dot products however many threads run them, so rows cost little up to 512 / 128 x 4 = 16; lin_bwd_w, the
// largest part of the backward pass, walks the workgroup's rows one after the other for each weight, so its time grows
// with G.  8 scenes are two full chunks, 13 workgroups at the workload's batch of 100 (one per CU, each with its 47 KB of
// a slice to leave and to be summed), and 50 688 B of LDS at the largest crowd.  Every access of the three helpers is a
// broadcast or runs along a row with lanes on consecutive elements: no bank conflicts at any row stride.
#include "dropout_hash.hpp"
#include "train_linear.hpp"     // NT, lin_fwd, lin_bwd_x, lin_bwd_w
#include "train_reduce.hpp"     // slice_floats, the reduce kernel

namespace {

constexpr int G = 8;                        // scenes of a workgroup
constexpr int H1 = 128, H2 = 64, H3 = 12;   // the hidden widths
constexpr int NMAX = MCN_MAX_HUMANS;

// the flat layout: mlp.0.weight, mlp.0.bias, mlp.3.*, mlp.6.*, mlp.8.*
struct MlpOffsets {
    int w0, b0, w1, b1, w2, b2, w3, b3, total;
};
__host__ __device__ inline MlpOffsets mlp_offsets(int N)
{
    MlpOffsets o;
    o.w0 = 0;
    o.b0 = o.w0 + H1 * 4 * N;
    o.w1 = o.b0 + H1;
    o.b1 = o.w1 + H2 * H1;
    o.w2 = o.b1 + H2;
    o.b2 = o.w2 + H3 * H2;
    o.w3 = o.b2 + H3;
    o.b3 = o.w3 + 2 * N * H3;
    o.total = o.b3 + 2 * N;                 // 538 N + 9164
    return o;
}

// per scene: float64 forward buffers, then float32 buffers
constexpr int SCENE_DOUBLES = H1 + H2 + H3 + 2 * NMAX;                                       // 268
constexpr int SCENE_FLOATS = 4 * NMAX + 2 * NMAX + 2 * NMAX + 3 * H1 + 3 * H2 + H3          // X Yt DZ, layers 1 and 2, A3
                             + H1 + H2 + H3;                                                // backward: T2 T0 T1
constexpr int LDS_DOUBLES = G * (SCENE_DOUBLES + SCENE_FLOATS / 2);
static_assert(SCENE_FLOATS % 2 == 0 && LDS_DOUBLES * 8 == 50688, "LDS of a workgroup");
static_assert(H1 >= 4 * NMAX && H1 <= DROPOUT_MAX_WIDTH, "H1d holds the loss terms; a layer fits the hash's unit range");

// dropout after a ReLU layer of width W, rows [R][W]: Yd *= m in float64, A = its float32 rounding, M = m in float32
__device__ void dropout_fwd(double *Yd, float *A, float *M, int R, int W, uint64_t key, int slot0, uint32_t T, double scale)
{
    for (int it = threadIdx.x; it < R * W; it += NT) {
        const int r = it / W, u = it - r * W;
        const double m = dropout_bits(key, slot0 + r, u) < T ? scale : 0.0;
        const double v = Yd[it] * m;
        Yd[it] = v;
        A[it] = (float)v;
        M[it] = (float)m;
    }
}

// dropout and the ReLU before it backwards: d = d * m, then 0 where the ReLU's output was <= 0
__device__ void dropout_bwd(float *D, const float *Hf, const float *M, int count)
{
    for (int it = threadIdx.x; it < count; it += NT) {
        const float v = D[it] * M[it];
        D[it] = Hf[it] <= 0.f ? 0.f : v;
    }
}

__global__ __launch_bounds__(NT) void mlp_world_loss_grad_kernel(const float *__restrict__ P, const float *__restrict__ cur,
                                                                 const float *__restrict__ nxt,
                                                                 const int64_t *__restrict__ rows, int B, int N,
                                                                 int want_grad, uint64_t seed, uint64_t step, uint32_t T,
                                                                 double scale, float *__restrict__ ws,
                                                                 double *__restrict__ ws_sums)
{
    __shared__ double lds[LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    const int R = min(G, B - b0);           // scenes of this group (the last group may be short)
    const int DI = 4 * N, DO = 2 * N;
    const MlpOffsets of = mlp_offsets(N);
    float *const gP = ws + (size_t)blockIdx.x * of.total;

    double *H1d = lds, *H2d = H1d + G * H1, *H3d = H2d + G * H2, *Zd = H3d + G * H3;
    float *at = reinterpret_cast<float *>(lds + G * SCENE_DOUBLES);
    auto take = [&at](int n) { float *q = at; at += n; return q; };
    float *X = take(G * DI), *Yt = take(G * DO), *DZ = take(G * DO);
    float *H1f = take(G * H1), *A1 = take(G * H1), *M1 = take(G * H1);
    float *H2f = take(G * H2), *A2 = take(G * H2), *M2 = take(G * H2);
    float *A3 = take(G * H3);
    float *T2 = take(G * H1), *T0 = take(G * H2), *T1 = take(G * H3);
    // the loss terms take the place of layer 1's float64 output, free once layer 2 has run
    double *SQ = H1d, *DZd = H1d + G * DO;

    // ---- gather: rows[b] (or b) picks the scene and its next velocities out of the pair memory
    for (int it = tid; it < R * DI; it += NT) {
        const int g = it / DI, k = it - g * DI;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[it] = cur[row * DI + k];
    }
    for (int it = tid; it < R * DO; it += NT) {
        const int g = it / DO, k = it - g * DO;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        Yt[it] = nxt[row * DO + k];
    }
    __syncthreads();

    // ---- forward (float64 from layer to layer; the float32 copies are what the backward pass reads).  Without a
    // gradient it is the eval-mode pass: no dropout.
    lin_fwd<float, false, true>(P + of.w0, DI, P + of.b0, X, DI, 1, H1d, H1, H1f, H1, R, DI, H1);
    __syncthreads();
    if (want_grad) {
        dropout_fwd(H1d, A1, M1, R, H1, dropout_key(seed, step, 0), b0, T, scale);
        __syncthreads();
    }
    lin_fwd<double, false, true>(P + of.w1, H1, P + of.b1, H1d, H1, 1, H2d, H2, H2f, H2, R, H1, H2);
    __syncthreads();
    if (want_grad) {
        dropout_fwd(H2d, A2, M2, R, H2, dropout_key(seed, step, 1), b0, T, scale);
        __syncthreads();
    }
    lin_fwd<double, false, true>(P + of.w2, H2, P + of.b2, H2d, H2, 1, H3d, H3, A3, H3, R, H2, H3);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w3, H3, P + of.b3, H3d, H3, 1, Zd, DO, nullptr, 0, R, H3, DO);
    __syncthreads();

    // ---- loss, all float64: out = tanh(z), the squared error, d loss / d z = 2 (out - y) / (B 2N) (1 - out^2); then
    // this group's sums in a fixed order -- per output over its scenes, and the squared errors over the outputs
    const double count = (double)B * (double)DO;
    for (int it = tid; it < R * DO; it += NT) {
        const double out = tanh(Zd[it]);
        const double d = out - (double)Yt[it];
        const double dz = 2.0 * d / count * (1.0 - out * out);
        SQ[it] = d * d;
        DZd[it] = dz;
        DZ[it] = (float)dz;
    }
    __syncthreads();
    const int nsums = 1 + DO;
    for (int k = tid; k < DO; k += NT) {
        double sq = 0.0, dsum = 0.0;
        for (int r = 0; r < R; ++r) {
            sq += SQ[r * DO + k];
            dsum += DZd[r * DO + k];
        }
        SQ[k] = sq;                                                     // (row 0 of SQ: read by this thread only so far)
        ws_sums[(size_t)nsums * blockIdx.x + 1 + k] = dsum;             // mlp.8.bias, before any float32 rounding
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int k = 0; k < DO; ++k) acc += SQ[k];
        ws_sums[(size_t)nsums * blockIdx.x] = acc;
    }
    if (!want_grad) return;                                             // forward only: the loss is all that is asked for

    // ---- backward (mlp.8.bias comes from the float64 sums above)
    lin_bwd_w(DZ, DO, A3, H3, 1, gP + of.w3, H3, nullptr, R, H3, DO);
    lin_bwd_x<false>(P + of.w3, H3, DZ, DO, T1, H3, A3, H3, R, H3, DO);
    __syncthreads();
    lin_bwd_w(T1, H3, A2, H2, 1, gP + of.w2, H2, gP + of.b2, R, H2, H3);
    lin_bwd_x<false>(P + of.w2, H2, T1, H3, T0, H2, nullptr, 0, R, H2, H3);
    __syncthreads();
    dropout_bwd(T0, H2f, M2, R * H2);
    __syncthreads();
    lin_bwd_w(T0, H2, A1, H1, 1, gP + of.w1, H1, gP + of.b1, R, H1, H2);
    lin_bwd_x<false>(P + of.w1, H1, T0, H2, T2, H1, nullptr, 0, R, H1, H2);
    __syncthreads();
    dropout_bwd(T2, H1f, M1, R * H1);
    __syncthreads();
    lin_bwd_w(T2, H1, X, DI, 1, gP + of.w0, DI, gP + of.b0, R, DI, H1);
}

}  // namespace

namespace mcn {

long mlp_world_train_param_count(int N) { return mlp_offsets(N).total; }

// the reduce kernel indexes the slices with an int
static bool groups_fit(long groups, int total) { return groups <= 0x7fffffffL / (total + 1); }

// one slice of every parameter's partial gradient per workgroup, then 1 + 2N float64 sums per workgroup; 0 for a batch
// that the launch refuses
long mlp_world_train_workspace_floats(int B, int N)
{
    const long groups = ((long)B + G - 1) / G;
    if (!groups_fit(groups, mlp_offsets(N).total)) return 0;
    return slice_floats(groups, mlp_offsets(N).total) + 2 * groups * (1 + 2 * N);
}

int launch_mlp_world_loss_grad(const float *params, const float *cur, const float *nxt, const int64_t *rows, int B, int N,
                               float drop_p, uint64_t seed, uint64_t step, void *workspace, float *grad, float *loss,
                               hipStream_t stream)
{
    const MlpOffsets of = mlp_offsets(N);
    const long groups = ((long)B + G - 1) / G;
    if (!groups_fit(groups, of.total)) return MCN_EINVAL;
    const double p = grad ? written_as(drop_p) : 0.0;                  // the decimal that was written: 0.1f means 0.1
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + slice_floats(groups, of.total));
    hipLaunchKernelGGL(mlp_world_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, cur, nxt, rows, B, N,
                       grad ? 1 : 0, seed, step, dropout_threshold(p), 1.0 / (1.0 - p), ws, ws_sums);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    return launch_train_grad_reduce(ws, ws_sums, groups, of.total, 1 + 2 * N, of.b3, 2 * N, (double)B * (double)(2 * N), grad,
                                    loss, stream);
}

int dropout_mask_host(uint64_t seed, uint64_t step, int layer, int B, int width, float p, uint8_t *keep)
{
    const uint64_t key = dropout_key(seed, step, layer);
    const uint32_t T = dropout_threshold(written_as(p));
    for (int b = 0; b < B; ++b)
        for (int u = 0; u < width; ++u) keep[(size_t)b * width + u] = dropout_bits(key, b, u) < T;
    return MCN_OK;
}

}  // namespace mcn
