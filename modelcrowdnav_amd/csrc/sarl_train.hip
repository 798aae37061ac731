// sarl_train.hip -- one training step of the SARL value network (policy/sarl.py: ValueNetwork, shipped dimensions,
// global state on) without autograd: MSE loss and its gradient for a mini-batch, and the SGD-momentum update.
//
//   sarl_loss_grad_kernel   one workgroup per G states (at most 8 rows, or one state).  It gathers its rows of the replay
//                           memory, runs the forward pass with every activation kept in LDS, forms its share of the
//                           loss and back-propagates through mlp3 (train_head.hpp: head_step), the pooling, the masked
//                           softmax, attention, the mean (global state), mlp2 and mlp1 (train_attention.hpp: the trunk).
//                           Its gradient of EVERY parameter goes into its own slice of the workspace: no atomics, no
//                           workgroup looks at another one's data.
//   train_grad_reduce_kernel (train_reduce.hpp) sums the slices in workgroup order into the flat gradient and
//                           writes the loss.
//   sgd_momentum_kernel     buf = momentum buf + grad, p = p - lr buf over the flat buffers.
//
// The three are ordered by the stream.  Parameters, gradient and momentum are flat float32 buffers in state_dict order
// (mlp1.0.weight, mlp1.0.bias, mlp1.2.*, mlp2.*, attention.*, mlp3.*), each weight row-major [out][in] as torch holds it.
// The backward pass is plain float32.  The forward pass accumulates and hands its activations from layer to layer in
// float64 (float32 copies of them stay in LDS for the backward pass), and the loss, d loss / d v and the sums over the
// workgroups are float64 rounded once: a value v, the loss and the gradient of mlp3.6.bias are then the float32 nearest to
// what float64 arithmetic gives, which single numbers need to stand a comparison with float64.  The semantics are those
// of torch autograd on ValueNetwork.forward: the softmax is the un-stabilised exp(s) (s != 0) / sum with the mask a
// constant, ReLU passes gradient where its output is > 0, and NaN goes where torch's goes (a state whose scores are all
// exactly 0 is 0 / 0).
#include "train_attention.hpp"  // the layer table and the trunk; NT, lin_fwd, lin_bwd_*
#include "train_head.hpp"       // mlp3 with the loss
#include "train_reduce.hpp"     // the grouping and the reduce kernel

namespace {

// LDS elements per row (one human of one state) and per state: the trunk's and, carved by the kernel after them, the
// gathered input, the joint state and the head's
constexpr int XS = 64;                   // row stride of the gathered input (input_dim <= 61)
constexpr int JOINT = 6 + 50;            // mlp3's input: [self state | pooled feature]
constexpr int ROW_FLOATS = XS + TRUNK_ROW_FLOATS;
constexpr int STATE_FLOATS = TRUNK_STATE_FLOATS + JOINT + HEAD_STATE_FLOATS;
constexpr int ROW_DOUBLES = TRUNK_ROW_DOUBLES;
constexpr int STATE_DOUBLES = TRUNK_STATE_DOUBLES + JOINT + HEAD_STATE_DOUBLES;
constexpr int LDS_DOUBLES = 20450;                                    // 163 600 B of the CU's 163 840
constexpr int ROWS64_IN_LDS = 20;        // up to here the rows' float64 buffers fit LDS too; above, they live in the workspace

TrainOffsets sarl_offsets(int D) { return train_offsets(D, JOINT, 1); }     // mlp3 on [self state | pooled feature] -> v
__device__ __forceinline__ HeadOffsets head_of(const TrainOffsets &of)      // mlp3's four layers, as head_step takes them
{
    HeadOffsets h;
    for (int l = 0; l < 4; ++l) h.w[l] = of.w[L3A + l], h.b[l] = of.b[L3A + l];
    return h;
}
bool rows64_in_lds(int N) { return N <= ROWS64_IN_LDS; }
bool group_fits(int G, int N)
{
    const long d = (long)G * STATE_DOUBLES + (rows64_in_lds(N) ? (long)G * N * ROW_DOUBLES : 0);
    const long f = (long)G * N * ROW_FLOATS + (long)G * STATE_FLOATS;
    return 8 * d + 4 * f <= 8L * LDS_DOUBLES && G * N <= 32;
}

__global__ __launch_bounds__(NT) void sarl_loss_grad_kernel(const float *__restrict__ P, TrainOffsets of, int D,
                                                            const float *__restrict__ states,
                                                            const float *__restrict__ values,
                                                            const int64_t *__restrict__ rows, int B, int N, int G,
                                                            float *__restrict__ ws, double *__restrict__ ws_sums,
                                                            double *__restrict__ ws_rows64)
{
    __shared__ double lds[LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    const int Gc = min(G, B - b0);          // states of this group (the last group may be short)
    const int R = Gc * N;                   // its rows
    float *const gP = ws + (size_t)blockIdx.x * of.total;

    const int Rcap = G * N;
    // float64 first (8-byte aligned), then the float32 buffers; the rows' float64 buffers of a large crowd are this
    // workgroup's own piece of the workspace instead
    double *st64 = lds;
    double *row64 = ws_rows64 ? ws_rows64 + (size_t)blockIdx.x * Rcap * ROW_DOUBLES : lds + (size_t)G * STATE_DOUBLES;
    float *at = reinterpret_cast<float *>(lds + (size_t)G * STATE_DOUBLES + (ws_rows64 ? 0 : (size_t)Rcap * ROW_DOUBLES));
    auto taked = [&st64](int n) { double *q = st64; st64 += n; return q; };
    auto take = [&at](int n) { float *q = at; at += n; return q; };
    float *X = take(Rcap * XS);
    const Trunk t = carve_trunk(st64, row64, at, G, Rcap);
    double *Jd = taked(G * JOINT);
    float *J = take(G * JOINT);
    const Head h = carve_head(st64, at, G);

    // ---- gather: rows[b] (or b) picks the state and its value out of the replay memory
    for (int it = tid; it < R * D; it += NT) {
        const int r = it / D, d = it - r * D, g = r / N, n = r - g * N;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[r * XS + d] = states[(row * N + n) * D + d];
    }
    if (tid < Gc) h.Yt[tid] = values[rows ? rows[b0 + tid] : (int64_t)(b0 + tid)];
    __syncthreads();

    // ---- forward (float64 from layer to layer; the float32 copies are what the backward pass reads)
    trunk_forward(P, of, X, XS, D, t, Gc, N, R);
    for (int it = tid; it < Gc * JOINT; it += NT) {                     // joint state: [self state | pooled feature]
        const int g = it / JOINT, j = it - g * JOINT;
        double acc;
        if (j < 6) acc = X[(g * N) * XS + j];
        else {
            acc = 0.0;
            for (int n = 0; n < N; ++n) acc = fma(t.WTd[g * N + n], t.FEATd[(g * N + n) * 52 + (j - 6)], acc);
        }
        Jd[it] = acc;
        J[it] = (float)acc;
    }
    __syncthreads();

    // ---- mlp3, forward and backward, with the loss: h.U1[g][6 + j] = d loss / d pooled
    head_step<double, true>(P, gP, head_of(of), Jd, JOINT, J, JOINT, JOINT, h, Gc, B, ws_sums);

    // ---- backward, the trunk: pooling, softmax, attention, the mean, mlp2, mlp1
    trunk_backward(P, gP, of, X, XS, D, h.U1 + 6, 152, t, Gc, N, R);
}

// torch.optim.SGD(momentum, dampening 0, no weight decay, not nesterov): buf.mul_(momentum).add_(grad), then
// p.add_(buf, alpha=-lr), which torch evaluates as one fused multiply-add
__global__ __launch_bounds__(256) void sgd_momentum_kernel(float *__restrict__ p, float *__restrict__ buf,
                                                           const float *__restrict__ grad, int64_t count, float lr,
                                                           float momentum)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) {
        const float b = momentum * buf[i] + grad[i];
        buf[i] = b;
        p[i] = fmaf(-lr, b, p[i]);
    }
}

}  // namespace

namespace mcn {

long sarl_train_param_count(int input_dim)
{
    return (input_dim == 13 || input_dim == 61) ? sarl_offsets(input_dim).total : -1;
}

// one slice of every parameter's partial gradient per workgroup, two float64 sums per workgroup, and for crowds above
// ROWS64_IN_LDS humans the float64 row buffers of each workgroup
long sarl_train_workspace_floats(int B, int N, int input_dim)
{
    const long groups = train_groups(B, N);
    const int G = group_states(N);
    return slice_floats(groups, (int)sarl_train_param_count(input_dim)) + 4 * groups +
           (rows64_in_lds(N) ? 0 : 2 * groups * G * N * ROW_DOUBLES);
}

int launch_sarl_loss_grad(const float *params, int input_dim, const float *states, const float *values,
                          const int64_t *rows, int B, int N, void *workspace, float *grad, float *loss,
                          hipStream_t stream)
{
    const TrainOffsets of = sarl_offsets(input_dim);
    const int G = group_states(N);
    const long groups = train_groups(B, N);
    if (!group_fits(G, N) || groups > 0x7fffffffL / (of.total + 1)) return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + slice_floats(groups, of.total));
    double *ws_rows64 = rows64_in_lds(N) ? nullptr : ws_sums + 2 * groups;
    hipLaunchKernelGGL(sarl_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, input_dim, states,
                       values, rows, B, N, G, ws, ws_sums, ws_rows64);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    return launch_train_grad_reduce(ws, ws_sums, groups, of.total, 2, of.b[L3D], 1, (double)B, grad, loss, stream);
}

int launch_sgd_momentum(float *params, float *momentum_buf, const float *grad, int64_t count, float lr, float momentum,
                        hipStream_t stream)
{
    const int64_t blocks = (count + 255) / 256;
    if (blocks > 0x7fffffffLL) return MCN_EINVAL;
    hipLaunchKernelGGL(sgd_momentum_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, params, momentum_buf, grad,
                       count, lr, momentum);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace mcn
