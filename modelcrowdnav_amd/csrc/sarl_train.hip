// sarl_train.hip -- one training step of the SARL value network (policy/sarl.py: ValueNetwork, shipped dimensions,
// global state on) without autograd: MSE loss and its gradient for a mini-batch, and the SGD-momentum update.
//
//   sarl_loss_grad_kernel   one workgroup per G states (at most 8 rows, or one state).  It gathers its rows of the replay
//                           memory, runs the forward pass with every activation kept in LDS, forms its share of the
//                           loss and back-propagates through mlp3, the pooling, the masked softmax, attention, the
//                           mean (global state), mlp2 and mlp1.  Its gradient of EVERY parameter goes into its own
//                           slice of the workspace: no atomics, no workgroup looks at another one's data.
//   sarl_grad_reduce_kernel sums the slices in workgroup order into the flat gradient and writes the loss.
//   sgd_momentum_kernel     buf = momentum buf + grad, p = p - lr buf over the flat buffers.
//
// The three are ordered by the stream.  Parameters, gradient and momentum are flat float32 buffers in state_dict order
// (mlp1.0.weight, mlp1.0.bias, mlp1.2.*, mlp2.*, attention.*, mlp3.*), each weight row-major [out][in] as torch holds it.
// The backward pass is plain float32.  The forward pass accumulates and hands its activations from layer to layer in
// float64 (float32 copies of them stay in LDS for the backward pass), and the loss, d loss / d v and the sums over the
// workgroups are float64 rounded once: a value v, the loss and the gradient of mlp3.6.bias are then the float32 nearest to
// what float64 arithmetic gives, which single numbers need to stand a comparison with float64.  The semantics are those of torch autograd on ValueNetwork.forward: the softmax is the
// un-stabilised exp(s) (s != 0) / sum with the mask a constant, ReLU passes gradient where its output is > 0, and NaN
// goes where torch's goes (a state whose scores are all exactly 0 is 0 / 0).
#include "launch.hpp"
#include "train_linear.hpp"    // NT, CH, lin_fwd, lin_bwd_x, lin_bwd_w

namespace {

constexpr int NLAYER = 11;
enum { L1A, L1B, L2A, L2B, LTA, LTB, LTC, L3A, L3B, L3C, L3D };

struct TrainOffsets {
    int w[NLAYER], b[NLAYER];   // float offsets of each layer's weight and bias in the flat buffers
    int total;
};

TrainOffsets train_offsets(int D)
{
    const int in[NLAYER] = {D, 150, 100, 100, 200, 100, 100, 56, 150, 100, 100};
    const int out[NLAYER] = {150, 100, 100, 50, 100, 100, 1, 150, 100, 100, 1};
    TrainOffsets t;
    int at = 0;
    for (int l = 0; l < NLAYER; ++l) {
        t.w[l] = at; at += in[l] * out[l];
        t.b[l] = at; at += out[l];
    }
    t.total = at;
    return t;
}

// LDS floats per row (one human of one state) and per state; the kernel carves its static array by the same numbers
constexpr int XS = 64;                   // row stride of the gathered input (input_dim <= 61)
constexpr int ROW_FLOATS = XS + 152 + 100 + 100 + 52 + 100 + 100 + 52 + 152 + 152 + 100 + 4;
constexpr int STATE_FLOATS = 100 + 56 + 152 + 100 + 100 + 152 + 152 + 100 + 3;
// float64 activations of the forward pass, per row (mlp1 output, feature, two layer buffers, score, e, weight) and per state
constexpr int ROW_DOUBLES = 100 + 52 + 152 + 100 + 3;
constexpr int STATE_DOUBLES = 100 + 56 + 152 + 100 + 100 + 1;
constexpr int LDS_DOUBLES = 20450;                                    // 163 600 B of the CU's 163 840
constexpr int ROWS64_IN_LDS = 20;        // up to here the rows' float64 buffers fit LDS too; above, they live in the workspace

// states per workgroup: up to 8 rows for small crowds, one state from 5 humans on (N <= 32 rows)
int group_states(int N) { return N > 4 ? 1 : 8 / N; }
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
    double *atd = lds;
    auto taked = [&atd](int n) { double *q = atd; atd += n; return q; };
    double *GMd = taked(G * 100), *Jd = taked(G * 56), *M1d = taked(G * 152), *M2d = taked(G * 100), *M3d = taked(G * 100);
    double *Vd = taked(G);
    if (ws_rows64) atd = ws_rows64 + (size_t)blockIdx.x * Rcap * ROW_DOUBLES;
    double *Hd = taked(Rcap * 100), *FEATd = taked(Rcap * 52), *Td = taked(Rcap * 152), *Ud = taked(Rcap * 100);
    double *Sd = taked(Rcap), *Ed = taked(Rcap), *WTd = taked(Rcap);
    float *at = reinterpret_cast<float *>(lds + (size_t)G * STATE_DOUBLES + (ws_rows64 ? 0 : (size_t)Rcap * ROW_DOUBLES));
    auto take = [&at](int n) { float *q = at; at += n; return q; };
    float *X = take(Rcap * XS), *H1 = take(Rcap * 152), *H = take(Rcap * 100), *F1 = take(Rcap * 100);
    float *FEAT = take(Rcap * 52), *A1 = take(Rcap * 100), *A2 = take(Rcap * 100), *DF = take(Rcap * 52);
    float *T0 = take(Rcap * 152), *T1 = take(Rcap * 152), *DH = take(Rcap * 100);
    float *S = take(Rcap), *WT = take(Rcap), *DWT = take(Rcap), *DS = take(Rcap);
    float *GM = take(G * 100), *J = take(G * 56), *M1 = take(G * 152), *M2 = take(G * 100), *M3 = take(G * 100);
    float *U0 = take(G * 152), *U1 = take(G * 152), *DG = take(G * 100);
    float *Yt = take(G), *DV = take(G), *ZS = take(G);

    // ---- gather: rows[b] (or b) picks the state and its value out of the replay memory
    for (int it = tid; it < R * D; it += NT) {
        const int r = it / D, d = it - r * D, g = r / N, n = r - g * N;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[r * XS + d] = states[(row * N + n) * D + d];
    }
    if (tid < Gc) Yt[tid] = values[rows ? rows[b0 + tid] : (int64_t)(b0 + tid)];
    __syncthreads();

    // ---- forward (float64 from layer to layer; the float32 copies are what the backward pass reads)
    lin_fwd<float, false, true>(P + of.w[L1A], D, P + of.b[L1A], X, XS, 1, Td, 152, H1, 152, R, D, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L1B], 150, P + of.b[L1B], Td, 152, 1, Hd, 100, H, 100, R, 150, 100);
    __syncthreads();
    for (int it = tid; it < Gc * 100; it += NT) {                       // global state: mean over the humans
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
    for (int it = tid; it < Gc * 56; it += NT) {                        // joint state: [self state | pooled feature]
        const int g = it / 56, j = it - g * 56;
        double acc;
        if (j < 6) acc = X[(g * N) * XS + j];
        else {
            acc = 0.0;
            for (int n = 0; n < N; ++n) acc = fma(WTd[g * N + n], FEATd[(g * N + n) * 52 + (j - 6)], acc);
        }
        Jd[it] = acc;
        J[it] = (float)acc;
    }
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L3A], 56, P + of.b[L3A], Jd, 56, 1, M1d, 152, M1, 152, Gc, 56, 150);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L3B], 150, P + of.b[L3B], M1d, 152, 1, M2d, 100, M2, 100, Gc, 150, 100);
    __syncthreads();
    lin_fwd<double, false, true>(P + of.w[L3C], 100, P + of.b[L3C], M2d, 100, 1, M3d, 100, M3, 100, Gc, 100, 100);
    __syncthreads();
    lin_fwd<double, false, false>(P + of.w[L3D], 100, P + of.b[L3D], M3d, 100, 1, Vd, 1, nullptr, 0, Gc, 100, 1);
    __syncthreads();

    // ---- loss: this group's sum of squared errors and of d loss / d v = 2 (v - y) / B, both float64
    if (tid == 0) {
        double acc = 0.0, dsum = 0.0;
        for (int g = 0; g < Gc; ++g) {
            const double d = Vd[g] - (double)Yt[g];
            const double dv = 2.0 * d / (double)B;
            acc += d * d;
            dsum += dv;
            DV[g] = (float)dv;
        }
        ws_sums[2 * blockIdx.x] = acc;
        ws_sums[2 * blockIdx.x + 1] = dsum;             // the gradient of mlp3.6.bias, before any float32 rounding
    }
    __syncthreads();

    // ---- backward: mlp3
    lin_bwd_w(DV, 1, M3, 100, 1, gP + of.w[L3D], 100, gP + of.b[L3D], Gc, 100, 1);
    lin_bwd_x<false>(P + of.w[L3D], 100, DV, 1, U0, 152, M3, 100, Gc, 100, 1);
    __syncthreads();
    lin_bwd_w(U0, 152, M2, 100, 1, gP + of.w[L3C], 100, gP + of.b[L3C], Gc, 100, 100);
    lin_bwd_x<false>(P + of.w[L3C], 100, U0, 152, U1, 152, M2, 100, Gc, 100, 100);
    __syncthreads();
    lin_bwd_w(U1, 152, M1, 152, 1, gP + of.w[L3B], 150, gP + of.b[L3B], Gc, 150, 100);
    lin_bwd_x<false>(P + of.w[L3B], 150, U1, 152, U0, 152, M1, 152, Gc, 150, 100);
    __syncthreads();
    lin_bwd_w(U0, 152, J, 56, 1, gP + of.w[L3A], 56, gP + of.b[L3A], Gc, 56, 150);
    lin_bwd_x<false>(P + of.w[L3A], 56, U0, 152, U1, 152, nullptr, 0, Gc, 56, 150);      // U1[g][6 + j] = d pooled
    __syncthreads();

    // ---- pooling and softmax
    for (int it = tid; it < R * 50; it += NT) {                         // d feature = weight * d pooled
        const int r = it / 50, j = it - r * 50;
        DF[r * 52 + j] = WT[r] * U1[(r / N) * 152 + 6 + j];
    }
    for (int r = tid; r < R; r += NT) {                                 // d weight = <d pooled, feature>
        float acc = 0.f;
        for (int j = 0; j < 50; ++j) acc = fmaf(U1[(r / N) * 152 + 6 + j], FEAT[r * 52 + j], acc);
        DWT[r] = acc;
    }
    __syncthreads();
    if (tid < Gc) {
        // w = e / sum, e = exp(s) mask.  Autograd's chain d e_n = d w_n / sum - sum_k d w_k e_k / sum^2,
        // d s_n = d e_n mask_n exp(s_n) is, with the factors collected, d s_n = w_n (d w_n - sum_k d w_k w_k): the same
        // numbers without the cancellation between two quotients, exactly 0 for a single human (w = 1) and for a masked
        // one (w = 0), and NaN for a state whose sum is 0 (w = NaN), as autograd's.
        float dot = 0.f;
        for (int n = 0; n < N; ++n) dot = fmaf(DWT[tid * N + n], WT[tid * N + n], dot);
        int m = -1;                                     // the participant (w != 0, or NaN) with the largest |d s|
        for (int n = 0; n < N; ++n) {
            const int r = tid * N + n;
            DS[r] = WT[r] * (DWT[r] - dot);
            if (!(WT[r] == 0.f) && (m < 0 || fabsf(DS[r]) > fabsf(DS[tid * N + m]))) m = n;
        }
        // The weights of a state sum to 1, so its d s sum to 0: a common shift of the scores (attention.4.bias) has no
        // gradient.  Rounding leaves 1e-10 of it.  The constraint is kept instead: the others are summed (float64, rounded
        // once) and the largest d s is set to minus that sum, which moves it by the rounding residue of the formula above;
        // the state's share of attention.4.bias is that sum plus that d s: 0 exactly, or NaN.
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
    lin_bwd_w(T1, 152, X, XS, 1, gP + of.w[L1A], D, gP + of.b[L1A], R, D, 150);
}

// grad[p] = sum over the workgroups' slices in index order; loss = (sum of their squared errors) / B.  The sums over the
// workgroups run in float64 and are rounded once: a few dozen additions per parameter, and the order stays fixed.
// mlp3.6.bias (index bias_v) is summed from the workgroups' float64 sums of d loss / d v.
__global__ __launch_bounds__(256) void sarl_grad_reduce_kernel(const float *__restrict__ ws,
                                                               const double *__restrict__ ws_sums, int groups, int total,
                                                               int bias_v, int B, float *__restrict__ grad,
                                                               float *__restrict__ loss)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < total && p != bias_v) {
        double acc = ws[p];
        for (int g = 1; g < groups; ++g) acc += (double)ws[(size_t)g * total + p];
        grad[p] = (float)acc;
    } else if (p == bias_v || p == total) {
        const int k = p == total ? 0 : 1;
        double acc = ws_sums[k];
        for (int g = 1; g < groups; ++g) acc += ws_sums[2 * g + k];
        if (k == 0) *loss = (float)(acc / (double)B);
        else grad[p] = (float)acc;
    }
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
    return (input_dim == 13 || input_dim == 61) ? train_offsets(input_dim).total : -1;
}

// workgroups of the loss/gradient kernel for a batch of B states of N humans
static long train_groups(int B, int N)
{
    const int G = group_states(N);
    return ((long)B + G - 1) / G;
}

// one slice of every parameter's partial gradient per workgroup (padded to whole float64s), two float64 sums per
// workgroup, and for crowds above ROWS64_IN_LDS humans the float64 row buffers of each workgroup
static long ws_slice_floats(long groups, int total) { return (groups * total + 1) / 2 * 2; }
long sarl_train_workspace_floats(int B, int N, int input_dim)
{
    const long groups = train_groups(B, N);
    const int G = group_states(N);
    return ws_slice_floats(groups, (int)sarl_train_param_count(input_dim)) + 4 * groups +
           (rows64_in_lds(N) ? 0 : 2 * groups * G * N * ROW_DOUBLES);
}

int launch_sarl_loss_grad(const float *params, int input_dim, const float *states, const float *values,
                          const int64_t *rows, int B, int N, void *workspace, float *grad, float *loss,
                          hipStream_t stream)
{
    const TrainOffsets of = train_offsets(input_dim);
    const int G = group_states(N);
    const long groups = train_groups(B, N);
    if (!group_fits(G, N) || groups > 0x7fffffffL / (of.total + 1)) return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + ws_slice_floats(groups, of.total));
    double *ws_rows64 = rows64_in_lds(N) ? nullptr : ws_sums + 2 * groups;
    hipLaunchKernelGGL(sarl_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, input_dim, states,
                       values, rows, B, N, G, ws, ws_sums, ws_rows64);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    hipLaunchKernelGGL(sarl_grad_reduce_kernel, dim3((unsigned)((of.total + 1 + 255) / 256)), dim3(256), 0, stream, ws,
                       ws_sums, (int)groups, of.total, of.b[L3D], B, grad, loss);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
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
