// kernels_pgo.hip -- the pose-graph optimiser on the device: ONE 1024-thread block per graph runs include/ssm/pgo_core.h's run<X> -- linearise, assemble,
// factor, solve, trial update, chi2 and the Levenberg decision of every iteration -- without a host round trip; n graphs are n blocks (ssm_pgo_optimize_many).
// Nothing waits across blocks.  The block is the executor X of the shared template: a loop over elements strides by the block's threads, a sync is
// __syncthreads (which also orders the block's global-memory traffic), a lane sum is pnp_core.h's tree -- thread t is lane t, the xor butterfly of its
// wave, the 16 wave sums added in order by every thread.  All arithmetic is f64; LDS holds the 16 wave sums only: the factor's column sweep reads each
// L entry once per column from the envelope in global memory (L2-resident for the graphs of a key-frame map), see DESIGN.md s.12.
#include "ssm_internal.h"
#include "../../include/ssm/pgo_core.h"

namespace {
struct DevExec {
    static __device__ __forceinline__ int tid() { return (int)threadIdx.x; }
    static __device__ __forceinline__ int nt() { return ssm_pgc::LANES; }
    static __device__ __forceinline__ void sync() { __syncthreads(); }
    static __device__ __forceinline__ long long clock() { return (long long)wall_clock64(); }
    template <class Term> static __device__ double lane_sum(int n, Term term)
    {
        __shared__ double grp[ssm_pgc::NGROUP];
        double acc = 0.0;
        for (int i = (int)threadIdx.x; i < n; i += ssm_pgc::LANES) acc += term(i);
#pragma unroll
        for (int s = 1; s < ssm_pgc::GROUP; s <<= 1) acc = acc + __shfl_xor(acc, s, ssm_pgc::GROUP);
        if ((threadIdx.x & (ssm_pgc::GROUP - 1)) == 0) grp[threadIdx.x / ssm_pgc::GROUP] = acc;
        __syncthreads();
        double r = grp[0];
#pragma unroll
        for (int g = 1; g < ssm_pgc::NGROUP; g++) r = r + grp[g];
        __syncthreads();                        // grp is free for the next sum
        return r;
    }
};
}  // namespace

// op 0: run(iterations); op 1: linearise + assemble at the current estimate; op 2: factor_solve(lambda) of the envelope and right-hand side in the view
__global__ void __launch_bounds__(ssm_pgc::LANES) pgo_kernel(const ssm_pgc::View* views, int iterations, int op, double lambda)
{
    const ssm_pgc::View v = views[blockIdx.x];
    if (op == 0) ssm_pgc::run<DevExec>(v, iterations);
    else if (op == 1) { if (v.na > 0 && v.nf > 0) ssm_pgc::linearize_assemble<DevExec>(v, false); }
    else if (v.nf > 0) ssm_pgc::factor_solve<DevExec>(v, lambda);
}

hipError_t k_pgo(const ssm_pgc::View* views, int n, int iterations, int op, double lambda, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(pgo_kernel, dim3(n), dim3(ssm_pgc::LANES), 0, s, views, iterations, op, lambda);
    return hipGetLastError();
}
