// value_train.hip -- one loss-and-gradient step, without autograd, of the two value networks that are a 150-100-100-1 MLP
// over a short input: CADRL's ValueNetwork (policy/cadrl.py: the MLP on one 13-wide row per state) and LSTM-RL's
// ValueNetwork1 (policy/lstm_rl.py: nn.LSTM(13, 50) over the N rows of a state in the order they are stored, then the MLP
// on [row 0's self state | h_N]), both with the shipped dimensions.  The scheme is sarl_train.hip's:
//
//   cadrl_loss_grad_kernel    one workgroup per CADRL_G = 8 states,
//   lstm_rl_loss_grad_kernel  one workgroup per G states of N rows (group_states: at most 8 rows, or one state).  Each
//                           gathers its rows of the replay memory, runs the forward pass with every activation kept in
//                           LDS, forms its share of the loss and back-propagates -- through the MLP and, for LSTM-RL, back
//                           through time.  Its gradient of EVERY parameter goes into its own slice of the workspace: no
//                           atomics, no workgroup looks at another one's data.
//   train_grad_reduce_kernel (train_reduce.hpp) sums the slices in workgroup order into the flat gradient and writes the
//                           loss.
//
// The update is sarl_train.hip's sgd_momentum_kernel.  Parameters and gradient are flat float32 buffers in state_dict
// order, each tensor row-major as torch holds it: value_network.{0,2,4,6}.{weight,bias} (27 401 floats), and for LSTM-RL
// the MLP FIRST -- mlp.{0,2,4,6}.{weight,bias}, lstm.weight_ih_l0 [200][13], lstm.weight_hh_l0 [200][50], lstm.bias_ih_l0,
// lstm.bias_hh_l0 (46 851 floats).  The forward pass accumulates and hands its activations on in float64 (float32 copies
// stay in LDS for the backward pass), sigmoid and tanh included; the loss, d loss / d v and the sums over the workgroups
// are float64 rounded once.  The backward pass is plain float32 with the formulas of torch autograd on the modules'
// forward: ReLU passes gradient where its output is > 0, sigmoid' = y (1 - y), tanh' = 1 - y^2, and NaN goes where torch's
// goes.  The LSTM is torch's: gates (i, f, g, o) = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh, c_t = f c_{t-1} + i g,
// h_t = o tanh(c_t), from zero h and c.
#include "train_head.hpp"      // the MLP both networks end in, with the loss; NT, lin_fwd, lin_bwd_x, lin_bwd_w
#include "train_reduce.hpp"    // the grouping and the reduce kernel

namespace {

// ---- CADRL: the MLP on one 13-wide row per state
constexpr int XS = 16;                  // row stride of the gathered input (13 columns)
constexpr int CADRL_G = 8;              // states of a workgroup
constexpr int CADRL_TOTAL = head_floats(13);
constexpr int CADRL_LDS_DOUBLES = CADRL_G * HEAD_STATE_DOUBLES + (CADRL_G * (XS + HEAD_STATE_FLOATS) + 1) / 2;

__global__ __launch_bounds__(NT) void cadrl_loss_grad_kernel(const float *__restrict__ P, HeadOffsets of,
                                                             const float *__restrict__ states,
                                                             const float *__restrict__ values,
                                                             const int64_t *__restrict__ rows, int B,
                                                             float *__restrict__ ws, double *__restrict__ ws_sums)
{
    __shared__ double lds[CADRL_LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * CADRL_G;
    const int Gc = min(CADRL_G, B - b0);    // states of this group (the last group may be short)
    float *const gP = ws + (size_t)blockIdx.x * CADRL_TOTAL;

    double *d64 = lds;                      // float64 first (8-byte aligned), then the float32 buffers
    float *f32 = reinterpret_cast<float *>(lds + CADRL_G * HEAD_STATE_DOUBLES);
    const Head h = carve_head(d64, f32, CADRL_G);
    float *X = f32;

    // ---- gather: rows[b] (or b) picks the state and its value out of the replay memory
    for (int it = tid; it < Gc * 13; it += NT) {
        const int g = it / 13, d = it - g * 13;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[g * XS + d] = states[row * 13 + d];
    }
    for (int g = tid; g < Gc; g += NT) h.Yt[g] = values[rows ? rows[b0 + g] : (int64_t)(b0 + g)];
    __syncthreads();

    head_step<float, false>(P, gP, of, X, XS, X, XS, 13, h, Gc, B, ws_sums);
}

// ---- LSTM-RL: the LSTM over a state's rows, then the MLP on [self state | h_N]
constexpr int HID = 50, GATES = 4 * HID, JOINT = 6 + HID;
constexpr int LSTM_HEAD = head_floats(JOINT);
constexpr int LSTM_WIH = LSTM_HEAD, LSTM_WHH = LSTM_WIH + GATES * 13, LSTM_BIH = LSTM_WHH + GATES * HID;
constexpr int LSTM_BHH = LSTM_BIH + GATES, LSTM_TOTAL = LSTM_BHH + GATES;

// LDS elements per row (one step of one state) and per state.  Float64: a row's gate pre-activations; a state's h, c and
// joint state.  Float32: a row's input, its gates (i, f, g, o -- overwritten by their gradients on the way back), c_t,
// tanh(c_t) and h_{t-1}; a state's joint state and the gradients by h and c that the recurrence carries backwards.
constexpr int ROW_DOUBLES = GATES;
constexpr int STATE_DOUBLES = HID + HID + JOINT + HEAD_STATE_DOUBLES;
constexpr int ROW_FLOATS = XS + GATES + HID + HID + HID;
constexpr int STATE_FLOATS = JOINT + HID + HID + HEAD_STATE_FLOATS;
constexpr int lstm_lds_doubles(int G, int N)
{
    return G * STATE_DOUBLES + G * N * ROW_DOUBLES + (G * N * ROW_FLOATS + G * STATE_FLOATS + 1) / 2;
}
// the largest group is one state of MCN_MAX_HUMANS rows (105 376 B of the CU's 163 840): every crowd fits LDS
constexpr int LSTM_LDS_DOUBLES = lstm_lds_doubles(1, MCN_MAX_HUMANS);
static_assert(lstm_lds_doubles(8, 1) <= LSTM_LDS_DOUBLES && lstm_lds_doubles(4, 2) <= LSTM_LDS_DOUBLES &&
              lstm_lds_doubles(2, 3) <= LSTM_LDS_DOUBLES && lstm_lds_doubles(2, 4) <= LSTM_LDS_DOUBLES &&
              8 * LSTM_LDS_DOUBLES <= 160 * 1024, "a group of states does not fit LDS");

__device__ __forceinline__ double sigmoid64(double x) { return 1.0 / (1.0 + exp(-x)); }   // exp(1000) = inf: 0, finite

__global__ __launch_bounds__(NT) void lstm_rl_loss_grad_kernel(const float *__restrict__ P, HeadOffsets of,
                                                               const float *__restrict__ states,
                                                               const float *__restrict__ values,
                                                               const int64_t *__restrict__ rows, int B, int N, int G,
                                                               float *__restrict__ ws, double *__restrict__ ws_sums)
{
    __shared__ double lds[LSTM_LDS_DOUBLES];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * G;
    const int Gc = min(G, B - b0);          // states of this group (the last group may be short)
    const int R = Gc * N;                   // its rows: r = g N + t
    float *const gP = ws + (size_t)blockIdx.x * LSTM_TOTAL;

    const int Rcap = G * N;
    double *d64 = lds;                      // float64 first (8-byte aligned), then the float32 buffers
    float *f32 = reinterpret_cast<float *>(lds + (size_t)G * STATE_DOUBLES + (size_t)Rcap * ROW_DOUBLES);
    auto taked = [&d64](int n) { double *q = d64; d64 += n; return q; };
    auto take = [&f32](int n) { float *q = f32; f32 += n; return q; };
    const Head h = carve_head(d64, f32, G);
    double *Hd = taked(G * HID), *Cd = taked(G * HID), *Jd = taked(G * JOINT), *GXd = taked(Rcap * GATES);
    float *X = take(Rcap * XS), *GT = take(Rcap * GATES), *C = take(Rcap * HID), *TC = take(Rcap * HID);
    float *HP = take(Rcap * HID), *J = take(G * JOINT), *DH = take(G * HID), *DC = take(G * HID);

    // ---- gather: rows[b] (or b) picks the state and its value out of the replay memory
    for (int it = tid; it < R * 13; it += NT) {
        const int r = it / 13, d = it - r * 13, g = r / N, n = r - g * N;
        const int64_t row = rows ? rows[b0 + g] : (int64_t)(b0 + g);
        X[r * XS + d] = states[(row * N + n) * 13 + d];
    }
    for (int g = tid; g < Gc; g += NT) h.Yt[g] = values[rows ? rows[b0 + g] : (int64_t)(b0 + g)];
    for (int it = tid; it < Gc * HID; it += NT) {                       // h_0 = c_0 = 0
        const int g = it / HID, u = it - g * HID;
        Hd[it] = 0.0;
        Cd[it] = 0.0;
        HP[(g * N) * HID + u] = 0.f;
    }
    __syncthreads();

    // ---- forward: the input's share of every step's gates at once, then N dependent steps
    lin_fwd<float, false, false>(P + LSTM_WIH, 13, P + LSTM_BIH, X, XS, 1, GXd, GATES, nullptr, 0, R, 13, GATES);
    __syncthreads();
    for (int t = 0; t < N; ++t) {
        // rows t, N + t, ...: one per state; GXd += W_hh h_{t-1}
        lin_fwd<double, true, false>(P + LSTM_WHH, HID, nullptr, Hd, HID, 1, GXd + t * GATES, N * GATES, nullptr, 0, Gc, HID,
                                     GATES);
        __syncthreads();
        for (int it = tid; it < Gc * HID; it += NT) {
            const int g = it / HID, u = it - g * HID, r = g * N + t;
            const double *pre = GXd + r * GATES;
            const float *bhh = P + LSTM_BHH;
            const double i = sigmoid64(pre[u] + (double)bhh[u]);
            const double f = sigmoid64(pre[HID + u] + (double)bhh[HID + u]);
            const double gg = tanh(pre[2 * HID + u] + (double)bhh[2 * HID + u]);
            const double o = sigmoid64(pre[3 * HID + u] + (double)bhh[3 * HID + u]);
            const double c = f * Cd[it] + i * gg;
            const double tc = tanh(c);
            const double hn = o * tc;
            Cd[it] = c;
            Hd[it] = hn;
            GT[r * GATES + u] = (float)i;
            GT[r * GATES + HID + u] = (float)f;
            GT[r * GATES + 2 * HID + u] = (float)gg;
            GT[r * GATES + 3 * HID + u] = (float)o;
            C[r * HID + u] = (float)c;
            TC[r * HID + u] = (float)tc;
            if (t + 1 < N) HP[(r + 1) * HID + u] = (float)hn;          // row r + 1 reads it as its h_{t-1}
        }
        __syncthreads();
    }
    for (int it = tid; it < Gc * JOINT; it += NT) {                     // joint state: [self state of row 0 | h_N]
        const int g = it / JOINT, j = it - g * JOINT;
        const double v = j < 6 ? (double)X[(g * N) * XS + j] : Hd[g * HID + (j - 6)];
        Jd[it] = v;
        J[it] = (float)v;
    }
    __syncthreads();

    // ---- the MLP, forward and backward: h.U1[g][6 + u] = d loss / d h_N
    head_step<double, true>(P, gP, of, Jd, JOINT, J, JOINT, JOINT, h, Gc, B, ws_sums);

    // ---- backward through time: GT[r] becomes the gradient by row r's gate pre-activations
    for (int it = tid; it < Gc * HID; it += NT) {
        const int g = it / HID, u = it - g * HID;
        DH[it] = h.U1[g * 152 + 6 + u];
        DC[it] = 0.f;
    }
    __syncthreads();
    for (int t = N - 1; t >= 0; --t) {
        for (int it = tid; it < Gc * HID; it += NT) {
            const int g = it / HID, u = it - g * HID, r = g * N + t;
            float *gt = GT + r * GATES;
            const float i = gt[u], f = gt[HID + u], gg = gt[2 * HID + u], o = gt[3 * HID + u], tc = TC[r * HID + u];
            const float cp = t > 0 ? C[(r - 1) * HID + u] : 0.f;
            const float dh = DH[it];
            const float dc = DC[it] + (dh * o) * (1.f - tc * tc);      // c_t feeds h_t and c_{t+1}
            gt[u] = (dc * gg) * ((1.f - i) * i);
            gt[HID + u] = (dc * cp) * ((1.f - f) * f);
            gt[2 * HID + u] = (dc * i) * (1.f - gg * gg);
            gt[3 * HID + u] = (dh * tc) * ((1.f - o) * o);
            DC[it] = dc * f;
        }
        __syncthreads();
        if (t > 0) {                                                    // d h_{t-1} = W_hh^T d gates_t
            lin_bwd_x<false>(P + LSTM_WHH, HID, GT + t * GATES, N * GATES, DH, HID, nullptr, 0, Gc, HID, GATES);
            __syncthreads();
        }
    }
    // the weights: sums over the (state, step) rows; both biases are the same sum, formed twice in the same order
    lin_bwd_w(GT, GATES, X, XS, 1, gP + LSTM_WIH, 13, gP + LSTM_BIH, R, 13, GATES);
    lin_bwd_w(GT, GATES, HP, HID, 1, gP + LSTM_WHH, HID, gP + LSTM_BHH, R, HID, GATES);
}

// what a launch needs of the workspace: one slice of every parameter's partial gradient per workgroup, then two float64
// sums per workgroup
long workspace_floats(long groups, int total) { return slice_floats(groups, total) + 4 * groups; }

}  // namespace

namespace mcn {

long cadrl_train_param_count() { return CADRL_TOTAL; }
long lstm_rl_train_param_count() { return LSTM_TOTAL; }

long cadrl_train_workspace_floats(int B) { return workspace_floats(((long)B + CADRL_G - 1) / CADRL_G, CADRL_TOTAL); }
long lstm_rl_train_workspace_floats(int B, int N) { return workspace_floats(train_groups(B, N), LSTM_TOTAL); }

int launch_cadrl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int B,
                           void *workspace, float *grad, float *loss, hipStream_t stream)
{
    const long groups = ((long)B + CADRL_G - 1) / CADRL_G;
    if (groups > 0x7fffffffL / (CADRL_TOTAL + 1)) return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + slice_floats(groups, CADRL_TOTAL));
    const HeadOffsets of = head_offsets(0, 13);
    hipLaunchKernelGGL(cadrl_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, states, values,
                       rows, B, ws, ws_sums);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    return launch_train_grad_reduce(ws, ws_sums, groups, CADRL_TOTAL, 2, of.b[3], 1, (double)B, grad, loss, stream);
}

int launch_lstm_rl_loss_grad(const float *params, const float *states, const float *values, const int64_t *rows, int B,
                             int N, void *workspace, float *grad, float *loss, hipStream_t stream)
{
    const int G = group_states(N);
    const long groups = train_groups(B, N);
    if (G * N > 32 || lstm_lds_doubles(G, N) > LSTM_LDS_DOUBLES || groups > 0x7fffffffL / (LSTM_TOTAL + 1))
        return MCN_EINVAL;
    float *ws = static_cast<float *>(workspace);
    double *ws_sums = reinterpret_cast<double *>(ws + slice_floats(groups, LSTM_TOTAL));
    const HeadOffsets of = head_offsets(0, JOINT);
    hipLaunchKernelGGL(lstm_rl_loss_grad_kernel, dim3((unsigned)groups), dim3(NT), 0, stream, params, of, states, values,
                       rows, B, N, G, ws, ws_sums);
    if (hipGetLastError() != hipSuccess) return MCN_ELAUNCH;
    return launch_train_grad_reduce(ws, ws_sums, groups, LSTM_TOTAL, 2, of.b[3], 1, (double)B, grad, loss, stream);
}

}  // namespace mcn
