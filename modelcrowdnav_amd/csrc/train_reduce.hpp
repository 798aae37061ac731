// train_reduce.hpp -- what every training step (sarl_train.hip, world_train.hip, world_mlp_train.hip, value_train.hip) does after its
// loss/gradient kernel: how a batch is grouped into workgroups, how their slices lie in the workspace, and the kernel that
// sums the slices in workgroup order into the flat gradient and writes the loss.
#pragma once
#include "launch.hpp"

namespace {

// ---- grouping: a workgroup takes G states (scenes) of N rows each -- up to 8 rows for small crowds, one state from 5
// humans on (N <= 32 rows) -- and leaves its partial gradient of every parameter in its own slice of the workspace
int group_states(int N) { return N > 4 ? 1 : 8 / N; }
long train_groups(int B, int N)
{
    const int G = group_states(N);
    return ((long)B + G - 1) / G;
}
// floats of all slices, padded to whole float64s: the workgroups' float64 sums follow them
long slice_floats(long groups, int total) { return (groups * total + 1) / 2 * 2; }

// ---- the sum over the workgroups.  A workgroup leaves `nsums` float64 sums at ws_sums[nsums g ..]: first its squared
// errors, then its d loss / d output, one per output.  loss = (sum of the squared errors) / divisor, and with a gradient
// asked for grad[p] = sum over the workgroups' slices in index order -- except the output layer's bias (the nbias indices
// from bias_at), which is summed from those float64 sums, before any float32 rounding.  All sums over the workgroups run in
// float64 in a fixed order and are rounded once.  Thread `total` has the loss; without a gradient thread 0 has it and
// nothing else is written.
__global__ __launch_bounds__(256) void train_grad_reduce_kernel(const float *__restrict__ ws,
                                                                const double *__restrict__ ws_sums, int groups, int total,
                                                                int nsums, int bias_at, int nbias, double divisor,
                                                                float *__restrict__ grad, float *__restrict__ loss)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int last = grad ? total : 0;
    if (p > last) return;
    double acc;
    if (p == last || (p >= bias_at && p < bias_at + nbias)) {
        const int k = p == last ? 0 : 1 + p - bias_at;
        acc = ws_sums[k];
        for (int g = 1; g < groups; ++g) acc += ws_sums[nsums * g + k];
    } else {
        acc = ws[p];
        for (int g = 1; g < groups; ++g) acc += (double)ws[(size_t)g * total + p];
    }
    if (p == last) *loss = (float)(acc / divisor);
    else grad[p] = (float)acc;
}

int launch_train_grad_reduce(const float *ws, const double *ws_sums, long groups, int total, int nsums, int bias_at,
                             int nbias, double divisor, float *grad, float *loss, hipStream_t stream)
{
    const unsigned blocks = grad ? (unsigned)((total + 1 + 255) / 256) : 1u;
    hipLaunchKernelGGL(train_grad_reduce_kernel, dim3(blocks), dim3(256), 0, stream, ws, ws_sums, (int)groups, total, nsums,
                       bias_at, nbias, divisor, grad, loss);
    return hipGetLastError() == hipSuccess ? MCN_OK : MCN_ELAUNCH;
}

}  // namespace
